"""Generate golden G12 (tests/golden/g12_track.npz): the reference's landmark fit on the synthetic identity of
tests/track_helpers.py, recorded so that the tests of instag_amd.track need no reference checkout.

Run in the build container only (needs the reference checkout; never on the GPU box), on the CPU:

    python tests/golden/make_golden_track.py

data_utils/face_tracking/{util,facemodel}.py are imported from the reference tree; their ``.cuda()`` calls are
neutralised inside this process (Tensor.cuda returns the tensor).  The synthetic model is written to a temporary
directory in the layout the reference's loader reads (with dummy texture fields, which the landmark fit never touches).
F = 6 frames, P = 5 candidates per contour slot, id_dim 100, exp_dim 79, focal 1000, 512 x 512, fp32 throughout.
Recorded: the landmarks of the identity, the perturbed start, get_3dlandmarks and forward_transform at the start, the
landmark loss, the autograd gradients of the joint loss, and the parameters after 25 iterations of the pose-only loop
body (Adam, lr 0.1) followed by 25 iterations of the joint loop body (a fresh id / exp Adam, the pose Adam carried over).
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import track_helpers as th  # noqa: E402

REF = "/root/reference"
SEED, F, P, FOCAL, ITERS = 12, 6, 5, 1000.0, 25


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, os.path.join(REF, "data_utils", "face_tracking"))
    import facemodel
    import util

    info, keys = th.model_arrays(SEED, P)
    n = info["mu_shape"].shape[0] // 3
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "3DMM_info.npy"), dict(info, b_tex=np.zeros((1, 3 * n)), mu_tex=np.zeros(3 * n),
                                                       sig_tex=np.ones(1)), allow_pickle=True)
        np.save(os.path.join(d, "keys_info.npy"), dict(keys, rigid_ids=np.arange(4)), allow_pickle=True)
        ref = facemodel.Face_3DMM(d, 100, 79, 1, n)
    for k in ("base_id", "base_exp", "mu", "sig_id", "sig_exp"):
        setattr(ref, k, getattr(ref, k).float())

    m = th.model(SEED, P)
    ident = th.identity(m, F, SEED, FOCAL)
    st = th.perturbed_state(m, ident, [FOCAL], SEED, dtype=torch.float32)
    lms = ident["lms"]
    cxy = torch.tensor((th.W / 2.0, th.H / 2.0), dtype=torch.float)
    focal = torch.tensor([FOCAL], dtype=torch.float)
    leaf = lambda t: t.detach().clone().contiguous().requires_grad_(True)
    id_para, exp_para, euler, trans = leaf(st.id), leaf(st.exp), leaf(st.pose[:, :3]), leaf(st.pose[:, 3:])
    rec = dict(lms=lms.numpy(), id0=st.id.numpy(), exp0=st.exp.numpy(), pose0=st.pose.numpy())

    def forward():
        geometry = ref.get_3dlandmarks(id_para.expand(F, -1), exp_para, euler, trans, focal, cxy)
        proj = util.forward_transform(geometry, euler, trans, focal, cxy)
        return geometry, proj, util.cal_lan_loss(proj[:, :, :2], lms)

    geometry, proj, loss_lan = forward()
    joint = loss_lan + torch.mean(id_para * id_para) * 0.5 + torch.mean(exp_para * exp_para) * 0.4
    grads = torch.autograd.grad(joint, [id_para, exp_para, euler, trans])
    rec.update(lands=geometry.detach().numpy(), proj=proj.detach().numpy(), loss_lan=loss_lan.detach().numpy(),
               g_id=grads[0].numpy(), g_exp=grads[1].numpy(),
               g_euler=grads[2].numpy(), g_trans=grads[3].numpy())

    optimizer_frame = torch.optim.Adam([euler, trans], lr=0.1)
    for _ in range(ITERS):
        loss = forward()[2]
        optimizer_frame.zero_grad()
        loss.backward()
        optimizer_frame.step()
    rec.update(pose_fit_euler=euler.detach().numpy().copy(), pose_fit_trans=trans.detach().numpy().copy(),
               pose_fit_last_loss=loss.detach().numpy())
    optimizer_idexp = torch.optim.Adam([id_para, exp_para], lr=0.1)
    for _ in range(ITERS):
        loss_lan = forward()[2]
        loss = loss_lan + torch.mean(id_para * id_para) * 0.5 + torch.mean(exp_para * exp_para) * 0.4
        optimizer_idexp.zero_grad()
        optimizer_frame.zero_grad()
        loss.backward()
        optimizer_idexp.step()
        optimizer_frame.step()
    rec.update(joint_fit_id=id_para.detach().numpy(), joint_fit_exp=exp_para.detach().numpy(),
               joint_fit_euler=euler.detach().numpy(), joint_fit_trans=trans.detach().numpy(),
               joint_fit_last_loss=loss_lan.detach().numpy())
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g12_track.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "bytes; loss_lan", float(rec["loss_lan"]), "->", float(rec["pose_fit_last_loss"]),
          "->", float(rec["joint_fit_last_loss"]))


if __name__ == "__main__":
    main()
