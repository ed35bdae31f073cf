"""Generate golden G13 (tests/golden/g13_photometric.npz): the reference's full-mesh geometry, texture, rotation, colour
and Laplacian losses, vertex normals and SH illumination on the synthetic mesh model of tests/photo_helpers.py, recorded
so that the tests of instag_amd.mesh_render need no reference checkout.

Run in the build container only (needs the reference checkout; never on the GPU box), on the CPU:

    python tests/golden/make_golden_photometric.py

data_utils/face_tracking/{util,facemodel,render_3dmm}.py are imported from the reference tree; their ``.cuda()`` calls are
neutralised inside this process (Tensor.cuda returns the tensor).  render_3dmm.py imports pytorch3d at its top, which is
not installed: ``sys.modules`` is seeded with empty stand-ins for those names, in this process only, to reach the two
pure-torch methods ``Render_3DMM.compute_normal`` (called on a plain object that carries tris and vert_tris: the
constructor would build pytorch3d's renderer) and ``Render_3DMM.Illumination_layer`` (static).  Nothing of pytorch3d runs.

Mesh 7 x 7 (seed 13), B = 4, id_dim 4, exp_dim 3, tex_dim 5, fp32 throughout.  Next to every recorded quantity ``<key>``
the generator writes ``spread_<key>``: |reference fp32 - this project's statement in fp64 on the same fp32 inputs|, the
fp32 rounding of the quantity, from which the test takes its bound where bit-equality is not asked.
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from instag_amd import mesh_render as mr  # noqa: E402
from tests import photo_helpers as ph  # noqa: E402

REF = "/root/reference"
N_GRID, SEED, B = 7, 13, 4


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return object


def inputs(m):
    sc = ph.scene(m, B, SEED)
    rng = np.random.default_rng(SEED + 7)
    f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    d = {k: sc[k].float() for k in ("id", "exp", "tex", "euler", "trans", "light")}
    d["pred"], d["gt"] = f(rng.uniform(0, 255, (B, 6, 8, 3))), f(rng.integers(0, 256, (B, 6, 8, 3)))
    d["mask"] = torch.as_tensor(rng.uniform(0, 1, (B, 6, 8)) > 0.4)
    return d


def statement(m, d, dtype):
    c = lambda t: t.to(dtype) if t.is_floating_point() else t
    d = {k: c(v) for k, v in d.items()}
    tris, vert_tris = m.topology_tensors("cpu")
    geo = mr.geometry_torch(m, d["id"].expand(B, -1), d["exp"])
    sub = mr.geometry_sub_torch(m, d["id"].expand(B, -1), d["exp"], m.rigid_ids)
    tex = mr.texture_torch(m, d["tex"].expand(B, -1))
    rott = mr.rott_torch(geo, d["euler"], d["trans"])
    normal = mr.vertex_normals_torch(rott, tris, vert_tris)
    rott_sub = mr.rott_torch(sub, d["euler"], d["trans"])
    return dict(geo=geo, geo_sub=sub, tex=tex, rott=rott, normal=normal, colour=mr.illumination_torch(tex, normal, d["light"]),
                col_loss=mr.color_loss_torch(d["pred"], d["gt"], d["mask"]),
                lap_loss=mr.lap_loss_torch(rott_sub.reshape(B, -1).permute(1, 0)))


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self
    for name in ("pytorch3d", "pytorch3d.structures", "pytorch3d.renderer", "pytorch3d.ops", "pytorch3d.renderer.blending"):
        sys.modules[name] = _Anything(name)
    sys.path.insert(0, os.path.join(REF, "data_utils", "face_tracking"))
    import facemodel
    import util
    import render_3dmm

    info, keys, topo = ph.model_arrays(N_GRID, SEED)
    m = ph.model(N_GRID, SEED)
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "3DMM_info.npy"), info, allow_pickle=True)
        np.save(os.path.join(tmp, "keys_info.npy"), keys, allow_pickle=True)
        ref = facemodel.Face_3DMM(tmp, m.id_dim, m.exp_dim, m.tex_dim, m.N)
    for k in ("base_id", "base_exp", "mu", "sig_id", "sig_exp", "base_tex", "mu_tex", "sig_tex"):
        setattr(ref, k, getattr(ref, k).float())
    d = inputs(m)
    holder = types.SimpleNamespace(tris=torch.as_tensor(topo["tris"]), vert_tris=torch.as_tensor(topo["vert_tris"]))
    ids = d["id"].expand(B, -1)
    geo = ref.forward_geo(ids, d["exp"])
    sub = ref.forward_geo_sub(ids, d["exp"], ref.rigid_ids)
    tex = ref.forward_tex(d["tex"].expand(B, -1))
    rott = util.forward_rott(geo, d["euler"], d["trans"])
    normal = render_3dmm.Render_3DMM.compute_normal(holder, rott)
    colour = render_3dmm.Render_3DMM.Illumination_layer(tex, normal, d["light"])
    rott_sub = util.forward_rott(sub, d["euler"], d["trans"])
    rec = dict(geo=geo, geo_sub=sub, tex=tex, rott=rott, normal=normal, colour=colour,
               col_loss=util.cal_col_loss(d["pred"], d["gt"], d["mask"]),
               lap_loss=util.cal_lap_loss([rott_sub.reshape(B, -1).permute(1, 0)], [1.0]))
    rec = {k: v.detach().numpy() for k, v in rec.items()}
    s64 = statement(m, d, torch.float64)
    out = {f"in_{k}": v.numpy() for k, v in d.items()}
    for k, v in rec.items():
        out[k] = v
        out[f"spread_{k}"] = np.float64(np.abs(v.astype(np.float64) - s64[k].numpy().reshape(v.shape)).max())
        print(f"{k}: |reference fp32 - statement fp64| = {float(out[f'spread_{k}']):.3e}   max |.| = {np.abs(v).max():.3e}")
    s32 = statement(m, d, torch.float32)
    for k, v in rec.items():
        print(f"{k}: fp32 statement bit-equal to the reference: {np.array_equal(s32[k].numpy().reshape(v.shape), v)}")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g13_photometric.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
