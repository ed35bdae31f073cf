"""Generate golden G10 (tests/golden/g10_dataset.npz): the reference's readCamerasFromTransforms on a tiny seeded
identity directory (6 train + 3 val frames, 24 x 20 pixels, lossless .png through its ``extension`` parameter).

Run in the build container only (needs the reference checkout and PIL; never on the GPU box), on the CPU:

    python tests/golden/make_golden_dataset.py

scene/dataset_readers.py is loaded from its file, the way make_golden.py loads the reference's modules; the modules
absent here (plyfile, librosa) and the reference's scene package (whose import pulls the CUDA extensions in) are
stubbed -- readCamerasFromTransforms uses none of them.  Stored: the input arrays (tests/dataset_helpers.make_arrays)
and, per call of tests/dataset_helpers.CALLS, what the reference made of them: image, background, the three masks,
auds, blink, au25, au_exp, the rects, mouth_bound, R, T, FovX / FovY, and the priors it loaded.
"""
import sys
sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree
import importlib.util
import os
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _reference_readers():
    for name in ("plyfile", "librosa"):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.PlyData = m.PlyElement = None
            sys.modules[name] = m
    scene = types.ModuleType("scene")
    scene.__path__ = []
    gm = types.ModuleType("scene.gaussian_model")
    gm.BasicPointCloud = tuple
    sys.modules["scene"], sys.modules["scene.gaussian_model"] = scene, gm
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("ref_dataset_readers", f"{REF}/scene/dataset_readers.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.path.remove(REF)
    return mod


def main():
    sys.path.insert(0, ROOT)
    from tests import dataset_helpers as D
    readers = _reference_readers()
    arrays = D.make_arrays()
    res = {f"in.{k}": np.asarray(v) for k, v in arrays.items()}
    with tempfile.TemporaryDirectory() as root:
        D.write_identity(root, arrays)
        for tag, split, n_views, audio in D.CALLS:
            cams = readers.readCamerasFromTransforms(root, f"transforms_{split}.json", False, extension=".png",
                                                     audio_file=os.path.join(root, audio) if audio else "",
                                                     audio_extractor="deepspeech", N_views=n_views, preload=True)
            td = [c.talking_dict for c in cams]
            out = dict(img_id=np.array([t["img_id"] for t in td]), image=np.stack([c.image for c in cams]),
                       background=np.stack([c.background for c in cams]),
                       face_mask=np.stack([t["face_mask"] for t in td]), hair_mask=np.stack([t["hair_mask"] for t in td]),
                       mouth_mask=np.stack([t["mouth_mask"] for t in td]),
                       auds=torch.stack([t["auds"] for t in td]).numpy(),
                       blink=np.array([float(t["blink"]) for t in td]), au25=np.array([t["au25"] for t in td], dtype=np.float64),
                       au_exp=torch.stack([t["au_exp"] for t in td]).numpy(),
                       lips_rect=np.array([t["lips_rect"] for t in td]), lhalf_rect=np.stack([t["lhalf_rect"] for t in td]),
                       mouth_bound=np.array([t["mouth_bound"] for t in td]), R=np.stack([c.R for c in cams]),
                       T=np.stack([c.T for c in cams]), FovX=np.array([c.FovX for c in cams]),
                       FovY=np.array([c.FovY for c in cams]))
            if "normal" in td[0]:
                out["normal"] = torch.stack([t["normal"] for t in td]).numpy()
                out["depth"] = torch.stack([t["depth"] for t in td]).numpy()
            assert out["image"].dtype == np.uint8 and out["background"].dtype == np.uint8 and out["face_mask"].dtype == bool
            print(tag, "frames", len(cams), "img_id", out["img_id"].tolist(), "priors", "normal" in out)
            res.update({f"{tag}.{k}": v for k, v in out.items()})
    path = f"{HERE}/g10_dataset.npz"
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
