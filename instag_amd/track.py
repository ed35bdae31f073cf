"""Track head pose from landmarks: the 3DMM landmark fit on the device (csrc/track.hip) and the transforms writer.

The reference's preprocessing runs ``data_utils/face_tracking/face_tracker.py`` on the ``ori_imgs/<i>.lms`` files and
writes ``track_params.pt``; ``data_utils/process.py:396-487`` (save_transforms) turns that into
``transforms_{train,val}.json``, the one file family ``dataset.open_identity`` reads that nothing here could write:

    model = Face3DMM.load("data_utils/face_tracking/3DMM")     # 3DMM_info.npy + keys_info.npy: not shipped here
    params = track_identity(path, model, "cuda")               # track_params.pt, transforms_train.json, transforms_val.json
    store, meta = open_identity(path, "train", "cuda")

Built: the focal search over nine candidates on every 40th frame (face_tracker.py:62-140), the coarse fit over all
frames (:145-205) and save_transforms.  About 44,000 Adam iterations of a tiny graph; here an iteration is one launch
for a whole pose-only segment and two launches per joint iteration, the nine focal candidates being nine groups of the
same launches.

``*_torch`` state in plain torch (any device, fp32 or fp64) what the kernels compute; they serve a CPU device and are
the reference of the GPU tests.

The two photometric stages that follow (face_tracker.py:207-406: light fit, frame-wise fine fit) are in mesh_render.py
and run with ``track_identity(..., photometric=True)``; without it the poses written are the reference's poses as they
stand at its line 205.

Stated deviations from the reference:
  * frames are the ``<i>.lms`` files in ascending numeric order (the reference walks range(frame_num), frame_num being
    the number of jpgs: the same frames whenever the ids are dense).
  * the kernels fold sig_id / sig_exp into the basis rows and rotate by Rz, Ry, Rx in turn instead of by their product:
    the same numbers up to fp32 rounding (DESIGN: parity table).
"""
from __future__ import annotations

import ctypes as C
import glob
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import check_arg

N_LMS = 68
N_SLOTS = 16
FOCALS = tuple(range(600, 1500, 100))
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
TRANS_Z0 = -7.0


# ---- the model -----------------------------------------------------------------------------------------------------------
class Face3DMM:
    """What facemodel.py:15-47 loads (texture, rigid_ids and the topology of render_3dmm.py:97-101 are optional keyword
    arguments: a model without them still serves the landmark fit): base_id [id_dim,3N], base_exp [exp_dim,3N], mu [3N] (mu_shape +
    mu_exp, centred per axis; all three / 1e5), sig_id, sig_exp, keyinds [68], left_contour, right_contour [8,P] (host,
    fp64 / int64).  ``points`` [M] lists the M = 68 + 16 P model points the landmark fit touches (keyinds, the left
    candidates slot-major, the right ones); only their basis rows go to a device."""

    def __init__(self, base_id, base_exp, mu, sig_id, sig_exp, keyinds, left_contour, right_contour, *, base_tex=None,
                 mu_tex=None, sig_tex=None, rigid_ids=None, tris=None, vert_tris=None):
        self.base_id, self.base_exp, self.mu = (np.asarray(a, dtype=np.float64) for a in (base_id, base_exp, mu))
        self.sig_id, self.sig_exp = np.asarray(sig_id, dtype=np.float64), np.asarray(sig_exp, dtype=np.float64)
        self.keyinds = np.asarray(keyinds, dtype=np.int64).reshape(-1)
        self.left_contour = np.asarray(left_contour, dtype=np.int64)
        self.right_contour = np.asarray(right_contour, dtype=np.int64)
        if self.keyinds.shape[0] != N_LMS:
            raise ValueError(f"keyinds must have 68 entries (the [:8] / [9:17] contour slots are fixed), got "
                             f"{self.keyinds.shape[0]}")
        if self.left_contour.ndim != 2 or self.left_contour.shape[0] != 8 or self.left_contour.shape != self.right_contour.shape:
            raise ValueError("left_contour and right_contour must be [8,P]")
        self.P = int(self.left_contour.shape[1])
        if not 1 <= self.P <= 64:
            raise ValueError("1 .. 64 candidates per contour slot")
        self.id_dim, self.exp_dim = int(self.base_id.shape[0]), int(self.base_exp.shape[0])
        if not (1 <= self.id_dim <= 128 and 1 <= self.exp_dim <= 128):
            raise ValueError("id_dim and exp_dim in 1 .. 128")
        n3 = self.mu.shape[0]
        if self.base_id.shape != (self.id_dim, n3) or self.base_exp.shape != (self.exp_dim, n3) or n3 % 3:
            raise ValueError("base_id [id_dim,3N], base_exp [exp_dim,3N], mu [3N]")
        if self.sig_id.shape != (self.id_dim,) or self.sig_exp.shape != (self.exp_dim,):
            raise ValueError("sig_id [id_dim], sig_exp [exp_dim]")
        self.points = np.concatenate([self.keyinds, self.left_contour.reshape(-1), self.right_contour.reshape(-1)])
        if self.points.min() < 0 or self.points.max() >= n3 // 3:
            raise ValueError("point index outside the model")
        self.M = int(self.points.shape[0])
        self._cache = {}
        self.N = n3 // 3
        # texture and topology (facemodel.py:30-35, :47; render_3dmm.py:97-101): only the photometric stages read them
        self.base_tex = self.mu_tex = self.sig_tex = self.rigid_ids = self.tris = self.vert_tris = None
        self.tex_dim = 0
        if base_tex is not None:
            self.base_tex, self.mu_tex = np.asarray(base_tex, dtype=np.float64), np.asarray(mu_tex, dtype=np.float64).reshape(-1)
            self.sig_tex = np.asarray(sig_tex, dtype=np.float64).reshape(-1)
            self.tex_dim = int(self.base_tex.shape[0])
            if self.base_tex.shape != (self.tex_dim, n3) or self.mu_tex.shape != (n3,) or self.sig_tex.shape != (self.tex_dim,):
                raise ValueError("base_tex [tex_dim,3N], mu_tex [3N], sig_tex [tex_dim]")
        if rigid_ids is not None:
            self.rigid_ids = np.asarray(rigid_ids, dtype=np.int64).reshape(-1)
            if self.rigid_ids.size == 0 or self.rigid_ids.min() < 0 or self.rigid_ids.max() >= self.N:
                raise ValueError("rigid_ids outside the model")
        if tris is not None:
            self.tris, self.vert_tris = np.asarray(tris, dtype=np.int64), np.asarray(vert_tris, dtype=np.int64)
            if self.tris.ndim != 2 or self.tris.shape[1] != 3 or self.tris.shape[0] < 1 or self.tris.min() < 0 or \
                    self.tris.max() >= self.N:
                raise ValueError("tris must be [T,3] with vertex indices in [0, N)")
            T = self.tris.shape[0]
            # vert_tris is used literally (render_3dmm.py:109): no padding rule is assumed, so every entry must name a triangle
            if self.vert_tris.ndim != 2 or self.vert_tris.shape[0] != self.N or self.vert_tris.shape[1] < 1 or \
                    self.vert_tris.min() < 0 or self.vert_tris.max() >= T:
                raise ValueError(f"vert_tris must be [N,M] with every entry in [0, {T})")

    has_texture = property(lambda self: self.base_tex is not None)
    has_topology = property(lambda self: self.tris is not None)

    @classmethod
    def from_arrays(cls, info: dict, keys: dict, id_dim: int = 100, exp_dim: int = 79, *, topo: dict = None,
                    tex_dim: int = 100):
        """info: the 3DMM_info dictionary (b_shape, mu_shape, b_exp, mu_exp, sig_shape, sig_exp; b_tex, mu_tex, sig_tex
        if it has them); keys: keys_info (keyinds, left_contour, right_contour; rigid_ids if it has them); topo:
        topology_info (tris, vert_tris) or None."""
        extra = {}
        if "b_tex" in info:
            extra.update(base_tex=np.asarray(info["b_tex"], dtype=np.float64)[:tex_dim], mu_tex=info["mu_tex"],
                         sig_tex=np.asarray(info["sig_tex"]).reshape(-1)[:tex_dim])
        if "rigid_ids" in keys:
            extra.update(rigid_ids=keys["rigid_ids"])
        if topo is not None:
            extra.update(tris=topo["tris"], vert_tris=topo["vert_tris"])
        mu = (np.asarray(info["mu_shape"], dtype=np.float64) + np.asarray(info["mu_exp"], dtype=np.float64)).reshape(-1, 3)
        mu = (mu - mu.mean(axis=0, keepdims=True)).reshape(-1)
        return cls(np.asarray(info["b_shape"], dtype=np.float64)[:id_dim] / 1e5,
                   np.asarray(info["b_exp"], dtype=np.float64)[:exp_dim] / 1e5, mu / 1e5,
                   np.asarray(info["sig_shape"]).reshape(-1)[:id_dim], np.asarray(info["sig_exp"]).reshape(-1)[:exp_dim],
                   keys["keyinds"], keys["left_contour"], keys["right_contour"], **extra)

    @classmethod
    def load(cls, directory, id_dim: int = 100, exp_dim: int = 79, *, tex_dim: int = 100):
        info = np.load(os.path.join(directory, "3DMM_info.npy"), allow_pickle=True).item()
        keys = np.load(os.path.join(directory, "keys_info.npy"), allow_pickle=True).item()
        topo = os.path.join(directory, "topology_info.npy")
        topo = np.load(topo, allow_pickle=True).item() if os.path.exists(topo) else None
        return cls.from_arrays(info, keys, id_dim, exp_dim, topo=topo, tex_dim=tex_dim)

    def full_tensors(self, device, dtype):
        """(base_id [I,3N], base_exp [E,3N], mu [3N], sig_id, sig_exp) of the whole mesh, for the photometric stages."""
        key = ("full", str(device), dtype)
        if key not in self._cache:
            self._cache[key] = tuple(torch.as_tensor(a, dtype=dtype, device=device) for a in
                                     (self.base_id, self.base_exp, self.mu, self.sig_id, self.sig_exp))
        return self._cache[key]

    def texture_tensors(self, device, dtype):
        """(base_tex [tex_dim,3N], mu_tex [3N], sig_tex [tex_dim])."""
        if not self.has_texture:
            raise ValueError("this Face3DMM was loaded without texture (b_tex, mu_tex, sig_tex of 3DMM_info)")
        key = ("tex", str(device), dtype)
        if key not in self._cache:
            self._cache[key] = tuple(torch.as_tensor(a, dtype=dtype, device=device) for a in
                                     (self.base_tex, self.mu_tex, self.sig_tex))
        return self._cache[key]

    def topology_tensors(self, device):
        """(tris [T,3], vert_tris [N,M]) int64."""
        if not self.has_topology:
            raise ValueError("this Face3DMM was loaded without topology (tris, vert_tris of topology_info.npy)")
        key = ("topo", str(device))
        if key not in self._cache:
            self._cache[key] = tuple(torch.as_tensor(a, dtype=torch.int64, device=device) for a in (self.tris, self.vert_tris))
        return self._cache[key]

    def _columns(self):
        return (3 * self.points[:, None] + np.arange(3)[None, :]).reshape(-1)

    def tensors(self, device, dtype):
        """(base_id [I,3M], base_exp [E,3M], mu [3M], sig_id, sig_exp) of the M points, for the statements."""
        key = ("plain", str(device), dtype)
        if key not in self._cache:
            c = self._columns()
            self._cache[key] = tuple(torch.as_tensor(a, dtype=dtype, device=device) for a in
                                     (self.base_id[:, c], self.base_exp[:, c], self.mu[c], self.sig_id, self.sig_exp))
        return self._cache[key]

    def device_tensors(self, device):
        """(basis [K,3M] with sig folded into the rows, its transpose [3M,K], mu [3M]) fp32 for the kernels."""
        key = ("hip", str(device))
        if key not in self._cache:
            c = self._columns()
            basis = np.concatenate([self.base_id[:, c] * self.sig_id[:, None], self.base_exp[:, c] * self.sig_exp[:, None]])
            f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(device)
            self._cache[key] = (f32(basis), f32(basis.T), f32(self.mu[c]))
        return self._cache[key]


def read_landmarks(ori_imgs_dir):
    """lms [F,68,2] float32 and the frame ids: the frames of ``ori_imgs_dir`` that have a ``<i>.lms`` file, in ascending
    numeric order (data_loader.py walks range(start, end) and skips the missing ones)."""
    ids = sorted(int(s) for s in (os.path.splitext(os.path.basename(p))[0]
                                  for p in glob.glob(os.path.join(ori_imgs_dir, "*.lms"))) if s.isdigit())
    if not ids:
        raise FileNotFoundError(f"no <number>.lms in {ori_imgs_dir}")
    lms = np.stack([np.loadtxt(os.path.join(ori_imgs_dir, f"{i}.lms"), dtype=np.float32) for i in ids])
    if lms.shape[1:] != (N_LMS, 2):
        raise ValueError(f"landmark files must hold 68 x 2 values, got {lms.shape[1:]}")
    return lms, ids


# ---- the state of a fit --------------------------------------------------------------------------------------------------
class TrackState:
    """Parameters, Adam moments and step counters of G groups of frames (group g: frames start[g] .. start[g+1], its own
    focal and id row).  ``state`` [G,8] fp64: {steps, beta1^steps, beta2^steps} of the pose optimizer, of the id / exp
    optimizer, and the learning rates of the running segment (include/instag_hip.h).  pose [F,6] = euler, trans."""

    TENSORS = ("id", "exp", "pose", "m_pose", "v_pose", "m_exp", "v_exp", "m_id", "v_id", "state")

    def __init__(self, lms, focals, start, h, w, id_dim, exp_dim, device, dtype):
        self.lms = torch.as_tensor(lms, dtype=dtype).to(device).contiguous()
        F = int(self.lms.shape[0])
        if tuple(self.lms.shape[1:]) != (N_LMS, 2) or F < 1:
            raise ValueError("lms [F,68,2], F >= 1")
        self.focals = [float(f) for f in focals]
        self.start = [int(s) for s in start]
        G = len(self.focals)
        if len(self.start) != G + 1 or self.start[0] != 0 or self.start[-1] != F or \
                any(b <= a for a, b in zip(self.start, self.start[1:])):
            raise ValueError("groups must cover frames 0 .. F and none may be empty")
        self.h, self.w, self.cx, self.cy = int(h), int(w), w / 2.0, h / 2.0
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=device)
        self.id, self.exp, self.pose = z(G, id_dim), z(F, exp_dim), z(F, 6)
        self.pose[:, 5] = TRANS_Z0
        self.m_pose, self.v_pose, self.m_exp, self.v_exp = z(F, 6), z(F, 6), z(F, exp_dim), z(F, exp_dim)
        self.m_id, self.v_id = z(G, id_dim), z(G, id_dim)
        self.state = torch.zeros(G, 8, dtype=torch.float64, device=device)
        self.state[:, [1, 2, 4, 5]] = 1.0
        self.loss = z(G)                                   # loss_lan of the last iteration run (before its step)
        self.frame_loss = z(F)
        self.sel = torch.zeros(F, N_SLOTS, dtype=torch.int32, device=device)

    G = property(lambda self: len(self.focals))
    F = property(lambda self: int(self.lms.shape[0]))
    euler = property(lambda self: self.pose[:, :3])
    trans = property(lambda self: self.pose[:, 3:])

    def fresh_idexp_optimizer(self):
        """optimizer_idexp is created anew in front of every joint loop; optimizer_frame is not."""
        for t in (self.m_exp, self.v_exp, self.m_id, self.v_id):
            t.zero_()
        self.state[:, 3], self.state[:, 4], self.state[:, 5] = 0.0, 1.0, 1.0

    def clone(self, device=None, dtype=None):
        other = object.__new__(TrackState)
        other.__dict__.update(self.__dict__)
        other.__dict__.pop("_ws", None)                  # (the kernels' workspace: per state)
        other.focals, other.start = list(self.focals), list(self.start)
        for k in self.TENSORS + ("lms", "loss", "frame_loss", "sel"):
            t = getattr(self, k)
            keep = k in ("state", "sel") or dtype is None
            setattr(other, k, t.detach().clone().to(device=device or t.device, dtype=t.dtype if keep else dtype))
        return other

    def frame_group(self):
        g = torch.zeros(self.F, dtype=torch.int64)
        for i, s in enumerate(self.start[1:-1]):
            g[s:] = i + 1
        return g.to(self.lms.device)


# ---- plain statements ----------------------------------------------------------------------------------------------------
def euler2rot_torch(euler):
    """[F,3] (theta, phi, psi) -> R [F,3,3] = Rx(theta) Ry(phi) Rz(psi) with the reference's signs (util.py:18-49)."""
    t, p, s = euler[:, 0], euler[:, 1], euler[:, 2]
    one, zero = torch.ones_like(t), torch.zeros_like(t)
    rows = lambda *r: torch.stack([torch.stack(x, dim=-1) for x in r], dim=-2)
    rx = rows((one, zero, zero), (zero, t.cos(), -t.sin()), (zero, t.sin(), t.cos()))
    ry = rows((p.cos(), zero, p.sin()), (zero, one, zero), (-p.sin(), zero, p.cos()))
    rz = rows((s.cos(), s.sin(), zero), (-s.sin(), s.cos(), zero), (zero, zero, one))
    return torch.bmm(rx, torch.bmm(ry, rz))


def project_torch(geometry, euler, trans, focal, cx, cy):
    """forward_transform (util.py:92-96): geometry [F,N,3] -> [F,N,3] = (-f X / Z + cx, f Y / Z + cy, Z) of R p + t.
    focal: a number or [F] / [F,1]."""
    rott = torch.bmm(euler2rot_torch(euler), geometry.permute(0, 2, 1)) + trans[:, :, None]
    X, Y, Z = rott[:, 0], rott[:, 1], rott[:, 2]
    if torch.is_tensor(focal):
        focal = focal.reshape(-1, 1)
    return torch.stack((-(focal * X) / Z + cx, (focal * Y) / Z + cy, Z), dim=2)


def candidates_torch(model, id_para, exp_para):
    """id_para, exp_para [F,*] -> the M candidate points [F,M,3] (facemodel.py:50-51, :64-68)."""
    base_id, base_exp, mu, sig_id, sig_exp = model.tensors(id_para.device, id_para.dtype)
    geo = torch.mm(id_para * sig_id, base_id) + torch.mm(exp_para * sig_exp, base_exp) + mu
    return geo.view(id_para.shape[0], model.M, 3)


def landmarks_torch(model, id_para, exp_para, euler, trans, focal, cx, cy, return_choice=False):
    """get_3dlandmarks (facemodel.py:49-120): the 68 model points [F,68,3] of every frame.  Landmarks 0..7 are the
    candidate of smallest projected x of the eight left contour rows, 9..16 the one of largest projected x of the right
    rows; among equal candidates the FIRST (lowest index) is taken, as torch.argmin / argmax do on the host.  The choice
    is an index: nothing is differentiated through it.  return_choice: also the [F,16] candidate indices."""
    F, P = id_para.shape[0], model.P
    geo = candidates_torch(model, id_para, exp_para)
    with torch.no_grad():
        px = project_torch(geo[:, N_LMS:], euler, trans, focal, cx, cy)[:, :, 0].reshape(F, N_SLOTS, P)
        choice = torch.cat((_first_extreme(px[:, :8], smallest=True), _first_extreme(px[:, 8:], smallest=False)), dim=1)
    picked = torch.gather(geo[:, N_LMS:].reshape(F, N_SLOTS, P, 3), 2,
                          choice[:, :, None, None].expand(F, N_SLOTS, 1, 3))[:, :, 0]
    lands = torch.cat((picked[:, :8], geo[:, 8:9], picked[:, 8:], geo[:, 17:N_LMS]), dim=1)
    return (lands, choice) if return_choice else lands


def _first_extreme(x, smallest):
    """Index of the first minimum (maximum) along the last axis, stated without relying on argmin's tie behaviour."""
    ext = x.min(dim=-1, keepdim=True).values if smallest else x.max(dim=-1, keepdim=True).values
    idx = torch.arange(x.shape[-1], device=x.device).expand_as(x)
    return torch.where(x == ext, idx, torch.full_like(idx, x.shape[-1])).min(dim=-1).values


def losses_torch(model, st: TrackState, id_para=None, exp=None, pose=None):
    """-> (loss_lan [G], joint loss [G], frame_loss [F] (sums of squared residuals), choice [F,16])."""
    id_para = st.id if id_para is None else id_para
    exp = st.exp if exp is None else exp
    pose = st.pose if pose is None else pose
    fg = st.frame_group()
    focal = torch.as_tensor(st.focals, dtype=pose.dtype, device=pose.device)[fg]
    lands, choice = landmarks_torch(model, id_para[fg], exp, pose[:, :3], pose[:, 3:], focal, st.cx, st.cy, True)
    proj = project_torch(lands, pose[:, :3], pose[:, 3:], focal, st.cx, st.cy)[:, :, :2]
    frame = ((proj - st.lms) ** 2).sum(dim=(1, 2))
    lan, joint = [], []
    for g in range(st.G):
        a, b = st.start[g], st.start[g + 1]
        lan.append(frame[a:b].sum() / (2 * N_LMS * (b - a)))
        joint.append(lan[-1] + 0.5 * (id_para[g] ** 2).mean() + 0.4 * (exp[a:b] ** 2).mean())
    return torch.stack(lan), torch.stack(joint), frame, choice


def loss_and_grads_torch(model, st: TrackState):
    """loss_lan [G] and the autograd gradients of the summed joint loss: {"id", "exp", "pose"}, plus frame_loss, choice."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (st.id, st.exp, st.pose)]
    lan, joint, frame, choice = losses_torch(model, st, *leaves)
    g = torch.autograd.grad(joint.sum(), leaves)
    return lan.detach(), dict(id=g[0], exp=g[1], pose=g[2]), frame.detach(), choice


def _adam_torch(p, g, m, v, b1t, b2t, lr):
    """torch.optim.Adam's single-tensor update (defaults), in p's dtype; step scalars in fp64."""
    m.lerp_(g, 1 - BETA1)
    v.mul_(BETA2).addcmul_(g, g, value=1 - BETA2)
    denom = (v.sqrt() / (1 - b2t) ** 0.5).add_(ADAM_EPS)
    p.addcdiv_(m, denom, value=-(lr / (1 - b1t)))


def _counters(st, cols, lr_pose, lr_idexp):
    """One step of the optimizers whose counters start at ``cols`` of the (group-independent) state row, on the host."""
    s = st._row
    for c in cols:
        s[c], s[c + 1], s[c + 2] = s[c] + 1.0, s[c + 1] * BETA1, s[c + 2] * BETA2
    s[6], s[7] = lr_pose, lr_idexp
    return s


def _with_host_counters(st, body, n):
    st._row = st.state[0].tolist()                          # one read; the loop itself never waits for the device
    for _ in range(n):
        body()
    st.state[:] = torch.tensor(st._row, dtype=torch.float64)
    del st._row
    return st


def fit_pose_torch(model, st: TrackState, n: int, lr: float):
    """n iterations of the pose-only loop body (face_tracker.py:85-99 / :162-172) at learning rate lr, in place."""
    def body():
        pose = st.pose.detach().clone().requires_grad_(True)
        lan, _, frame, choice = losses_torch(model, st, pose=pose)
        (g,) = torch.autograd.grad(lan.sum(), [pose])
        s = _counters(st, (0,), lr, lr)
        _adam_torch(st.pose, g, st.m_pose, st.v_pose, s[1], s[2], lr)
        st.loss, st.frame_loss, st.sel = lan.detach(), frame.detach(), choice.to(torch.int32)
    return _with_host_counters(st, body, n)


def fit_joint_torch(model, st: TrackState, n: int, lr_pose: float, lr_idexp: float):
    """n iterations of the joint loop body (face_tracker.py:104-121 / :182-196), in place."""
    def body():
        lan, g, frame, choice = loss_and_grads_torch(model, st)
        s = _counters(st, (0, 3), lr_pose, lr_idexp)
        _adam_torch(st.id, g["id"], st.m_id, st.v_id, s[4], s[5], lr_idexp)
        _adam_torch(st.exp, g["exp"], st.m_exp, st.v_exp, s[4], s[5], lr_idexp)
        _adam_torch(st.pose, g["pose"], st.m_pose, st.v_pose, s[1], s[2], lr_pose)
        st.loss, st.frame_loss, st.sel = lan, frame, choice.to(torch.int32)
    return _with_host_counters(st, body, n)


# ---- schedules -----------------------------------------------------------------------------------------------------------
def _segments(lrs):
    """Per-iteration learning rates -> [(n, lr)] runs."""
    out = []
    for lr in lrs:
        if out and out[-1][1] == lr:
            out[-1][0] += 1
        else:
            out.append([1, lr])
    return [(n, lr) for n, lr in out]


def coarse_schedule(iters=(1500, 2000)):
    """The coarse stage's (pose segments, joint segments): a change takes effect AFTER the step of the iteration that
    triggers it (face_tracker.py:173-175, :199-203).  Defaults: 1,001 steps at 1 then 499 at 0.1; 1,001 at 0.1 then 999
    at 0.02."""
    pose = [1.0 if i <= 1000 else 0.1 for i in range(iters[0])]
    joint, lr = [], 0.1
    for i in range(iters[1]):
        joint.append(lr)
        if i % 1000 == 0 and i >= 1000:
            lr = lr * 0.2
    return _segments(pose), _segments(joint)


def focal_schedule(iters=(2000, 2500)):
    """The focal search's: 2,000 steps at 0.1; 1,501 at 0.1 then 999 at 0.02 (face_tracker.py:126-130)."""
    joint, lr = [], 0.1
    for i in range(iters[1]):
        joint.append(lr)
        if i % 1500 == 0 and i >= 1500:
            lr = lr * 0.2
    return _segments([0.1] * iters[0]), _segments(joint)


def _run_stage(fit_pose, fit_joint, st, schedule):
    pose_segments, joint_segments = schedule
    for n, lr in pose_segments:
        fit_pose(st, n, lr)
    st.fresh_idexp_optimizer()
    for n, lr in joint_segments:
        fit_joint(st, n, lr, lr)
    return st


def _pick_focal(focals, losses):
    best, best_loss = None, 1e5                           # arg_landis = 1e5; strict <, ascending focal order
    for f, l in zip(focals, losses):
        if l < best_loss:
            best, best_loss = f, l
    if best is None:
        raise RuntimeError(f"no focal candidate reached a landmark loss below 1e5: {losses}")
    return best


def _focal_state(model, lms, h, w, focals, every, device, dtype):
    sel = torch.as_tensor(lms)[::every]
    n = int(sel.shape[0])
    return TrackState(sel.repeat(len(focals), 1, 1), focals, [n * i for i in range(len(focals) + 1)], h, w,
                      model.id_dim, model.exp_dim, device, dtype)


def search_focal_torch(model, lms, h, w, focals=FOCALS, every=40, iters=(2000, 2500), device="cpu", dtype=torch.float32):
    """-> (best focal, [loss_lan per focal]): every candidate fitted on every ``every``-th frame."""
    st = _focal_state(model, lms, h, w, focals, every, device, dtype)
    _run_stage(lambda s, n, lr: fit_pose_torch(model, s, n, lr), lambda s, n, a, b: fit_joint_torch(model, s, n, a, b), st,
               focal_schedule(iters))
    losses = [float(x) for x in st.loss]
    return _pick_focal(list(focals), losses), losses


def coarse_fit_torch(model, lms, focal, h, w, iters=(1500, 2000), device="cpu", dtype=torch.float32):
    st = TrackState(lms, [focal], [0, len(lms)], h, w, model.id_dim, model.exp_dim, device, dtype)
    return _run_stage(lambda s, n, lr: fit_pose_torch(model, s, n, lr),
                      lambda s, n, a, b: fit_joint_torch(model, s, n, a, b), st, coarse_schedule(iters))


def _params(st, focal):
    return {"id": st.id.detach().float().cpu(), "exp": st.exp.detach().float().cpu(),
            "euler": st.pose[:, :3].detach().float().cpu().contiguous(),
            "trans": st.pose[:, 3:].detach().float().cpu().contiguous(),
            "focal": torch.tensor([float(focal)], dtype=torch.float32)}


def track_torch(model, lms, h, w, focals=FOCALS, every=40, focal_iters=(2000, 2500), coarse_iters=(1500, 2000),
                device="cpu", dtype=torch.float32):
    """The landmark stages end to end -> {"id" [1,I], "exp" [F,E], "euler" [F,3], "trans" [F,3], "focal" [1]}."""
    focal, _ = search_focal_torch(model, lms, h, w, focals, every, focal_iters, device, dtype)
    return _params(coarse_fit_torch(model, lms, focal, h, w, coarse_iters, device, dtype), focal)


# ---- the kernels ---------------------------------------------------------------------------------------------------------
class LandmarkTracker:
    """The fit on a HIP device.  States are TrackState objects (fp32, on the device); every method works in place and
    returns the state, so segments chain: ``fit_pose(st, 25, 0.1); fit_pose(st, 15, 0.1)`` is bit-identical to
    ``fit_pose(st, 40, 0.1)``."""

    def __init__(self, model: Face3DMM, device="cuda"):
        self.model, self.device = model, torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("LandmarkTracker runs on a HIP device; the *_torch functions serve any other")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.basis, self.basis_t, self.mu = model.device_tensors(self.device)
        self.max_groups = int(_lib.lib().instag_track_max_groups())

    def init_state(self, lms, focals, h, w, start=None) -> TrackState:
        start = [0, len(lms)] if start is None else start
        return TrackState(lms, focals, start, h, w, self.model.id_dim, self.model.exp_dim, self.device, torch.float32)

    def _args(self, st, grads=None):
        m, F = self.model, st.F
        ws = getattr(st, "_ws", None)
        if ws is None:
            ws = st._ws = (torch.empty(F, 3 * m.M, dtype=torch.float32, device=self.device),
                           torch.empty(F, m.id_dim, dtype=torch.float32, device=self.device))
        a = _lib.TrackArgs()
        for k, t in dict(basis=self.basis, basis_t=self.basis_t, mu=self.mu, lms=st.lms, id=st.id, exp=st.exp, pose=st.pose,
                         m_pose=st.m_pose, v_pose=st.v_pose, m_exp=st.m_exp, v_exp=st.v_exp, m_id=st.m_id, v_id=st.v_id,
                         state=st.state, geo=ws[0], did=ws[1], frame_loss=st.frame_loss, loss=st.loss, sel=st.sel).items():
            if t.device != self.device or not t.is_contiguous() or t.dtype not in (torch.float32, torch.float64, torch.int32):
                raise ValueError(f"track: {k} must be a contiguous tensor on {self.device}")
            setattr(a, k, t.data_ptr())
        if grads is not None:
            a.g_id, a.g_exp, a.g_pose = (g.data_ptr() for g in grads)
        starts, focals = (_lib.i32 * (st.G + 1))(*st.start), (_lib.f32 * st.G)(*st.focals)
        a.group_start, a.focal = C.addressof(starts), C.addressof(focals)
        a.G, a.F, a.id_dim, a.exp_dim, a.P, a.n_landmarks = st.G, F, m.id_dim, m.exp_dim, m.P, N_LMS
        a.cx, a.cy = st.cx, st.cy
        return a, (starts, focals)

    def geometry(self, st):
        """The candidate points [F,M,3] of the state's id / exp."""
        a, keep = self._args(st)
        with torch.cuda.device(self.device):
            check_arg(_lib.lib().instag_track_geometry(C.byref(a), _lib.current_stream()), "track_geometry")
        return st._ws[0].view(st.F, self.model.M, 3).clone()

    def fit_pose(self, st, n: int, lr: float):
        a, keep = self._args(st)
        with torch.cuda.device(self.device):
            check_arg(_lib.lib().instag_track_fit_pose(C.byref(a), int(n), float(lr), _lib.current_stream()), "track_fit_pose")
        return st

    def fit_joint(self, st, n: int, lr_pose: float, lr_idexp: float):
        a, keep = self._args(st)
        with torch.cuda.device(self.device):
            check_arg(_lib.lib().instag_track_fit_joint(C.byref(a), int(n), float(lr_pose), float(lr_idexp),
                                                       _lib.current_stream()), "track_fit_joint")
        return st

    def loss_and_grads(self, st):
        """loss_lan [G] and {"id", "exp", "pose"}: the gradients of the summed joint loss; st.frame_loss and st.sel are
        refreshed, nothing else changes."""
        grads = (torch.empty_like(st.id), torch.empty_like(st.exp), torch.empty_like(st.pose))
        a, keep = self._args(st, grads)
        with torch.cuda.device(self.device):
            check_arg(_lib.lib().instag_track_loss_grad(C.byref(a), _lib.current_stream()), "track_loss_grad")
        return st.loss.clone(), dict(id=grads[0], exp=grads[1], pose=grads[2])

    def search_focal(self, lms, h, w, focals=FOCALS, every=40, iters=(2000, 2500)):
        """-> (best focal, [loss_lan per focal]); the candidates are groups of the same launches, max_groups at a time."""
        focals, losses = list(focals), []
        for i in range(0, len(focals), self.max_groups):
            st = _focal_state(self.model, lms, h, w, focals[i:i + self.max_groups], every, self.device, torch.float32)
            _run_stage(self.fit_pose, self.fit_joint, st, focal_schedule(iters))
            losses += [float(x) for x in st.loss.cpu()]
        return _pick_focal(focals, losses), losses

    def coarse_fit(self, lms, focal, h, w, iters=(1500, 2000)):
        st = self.init_state(lms, [focal], h, w)
        return _run_stage(self.fit_pose, self.fit_joint, st, coarse_schedule(iters))


# ---- a directory ---------------------------------------------------------------------------------------------------------
def save_transforms(path, params, h, w):
    """transforms_train.json / transforms_val.json of ``path`` from {"focal", "euler", "trans"} (process.py:396-487):
    trans / 10, the pose [R^T | -R^T t], frames 0 .. int(F 10 / 11) for training and the rest for validation."""
    euler = torch.as_tensor(params["euler"], dtype=torch.float32).cpu()
    trans = torch.as_tensor(params["trans"], dtype=torch.float32).cpu() / 10.0
    n = int(euler.shape[0])
    rot_inv = euler2rot_torch(euler).permute(0, 2, 1)
    trans_inv = -torch.bmm(rot_inv, trans.unsqueeze(2))
    split = int(n * 10 / 11)
    for name, ids in (("train", range(0, split)), ("val", range(split, n))):
        frames = []
        for i in ids:
            pose = torch.eye(4, dtype=torch.float32)
            pose[:3, :3], pose[:3, 3] = rot_inv[i], trans_inv[i, :, 0]
            frames.append({"img_id": i, "aud_id": i, "transform_matrix": pose.numpy().tolist()})
        contents = {"focal_len": float(torch.as_tensor(params["focal"]).reshape(-1)[0]), "cx": float(w / 2.0),
                    "cy": float(h / 2.0), "frames": frames}
        with open(os.path.join(path, f"transforms_{name}.json"), "w") as fp:
            json.dump(contents, fp, indent=2, separators=(",", ": "))


def _image_size(ori_imgs_dir):
    from PIL import Image
    jpgs = sorted(glob.glob(os.path.join(ori_imgs_dir, "*.jpg")))
    if not jpgs:
        raise FileNotFoundError(f"no image in {ori_imgs_dir} to read the size from: pass h and w")
    with Image.open(jpgs[0]) as im:
        return im.height, im.width


def track_identity(path, model, device="cuda", write=True, h=None, w=None, focals=FOCALS, every=40,
                   focal_iters=(2000, 2500), coarse_iters=(1500, 2000), photometric=False, photo_batch=32, light_iters=71,
                   fine_iters=50, **render_settings):
    """ori_imgs/<i>.lms of ``path`` -> {"id" [1,I], "exp" [F,E], "euler" [F,3], "trans" [F,3], "focal" [1]} (CPU fp32:
    the keys and shapes of the reference's track_params.pt).  ``write``: also track_params.pt and the two transforms
    files.  h, w: the image size (default: read from the first ori_imgs/*.jpg).  The iteration counts default to the
    reference's; a CPU device runs the plain statements.  ``photometric``: also the light fit and the frame-wise fine fit
    against ``ori_imgs/<i>.jpg`` (mesh_render.py; face_tracker.py:207-406), which need a model with texture, rigid_ids and
    topology and at least ``photo_batch`` frames; ``render_settings`` (sigma, gamma, blur_radius, ...) go to the renderer."""
    ori = os.path.join(path, "ori_imgs")
    lms, frame_ids = read_landmarks(ori)
    if photometric:
        from . import mesh_render
        if not (model.has_texture and model.has_topology) or model.rigid_ids is None:
            raise ValueError("photometric=True needs a Face3DMM with texture (b_tex, mu_tex, sig_tex), rigid_ids and topology "
                             "(topology_info.npy)")
        if len(frame_ids) < photo_batch:
            raise ValueError(f"photometric=True needs at least {photo_batch} frames, got {len(frame_ids)}")
        images = mesh_render.jpg_loader(ori, frame_ids)
    if h is None or w is None:
        h, w = _image_size(ori)
    device = torch.device(device)
    if device.type == "cuda":
        tracker = LandmarkTracker(model, device)
        focal, _ = tracker.search_focal(lms, h, w, focals, every, focal_iters)
        params = _params(tracker.coarse_fit(lms, focal, h, w, coarse_iters), focal)
    else:
        params = track_torch(model, lms, h, w, focals, every, focal_iters, coarse_iters, device)
    if photometric:
        params = mesh_render.refine(model, params, lms, images, h, w, device, photo_batch, light_iters, fine_iters,
                                    **render_settings)
    if write:
        torch.save(params, os.path.join(path, "track_params.pt"))
        save_transforms(path, params, h, w)
    return params
