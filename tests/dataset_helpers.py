"""The tiny processed-identity directory of golden G10 (tests/golden/g10_dataset.npz): its seeded content as arrays, and
the writer that lays the arrays out as the files the reference's preprocessing produces.  Used by the generator
(tests/golden/make_golden_dataset.py) and by tests/test_dataset_host.py, which rebuilds the directory from the arrays
the golden recorded."""
import json
import os

import numpy as np

H, W = 20, 24
TRAIN_IDS, VAL_IDS = (0, 1, 2, 3, 4, 5), (6, 7, 8)
T_AUDIO = 10
# the calls the golden records: (tag, split, n_views, driving audio file inside the directory or '')
CALLS = (("train", "train", -1, ""), ("val", "val", -1, ""), ("train4", "train", 4, ""), ("val_audio", "val", -1, "drive.npy"))
PARSING = np.array([(0, 0, 255), (0, 0, 0), (100, 100, 100), (255, 255, 255), (0, 0, 254), (100, 100, 99), (0, 0, 1),
                    (1, 0, 255), (255, 0, 0)], dtype=np.uint8)


def make_arrays(seed=10):
    rng = np.random.default_rng(seed)
    ids = TRAIN_IDS + VAL_IDS
    n = len(ids)
    a = dict(gt=rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), torso=rng.integers(0, 256, (n, H, W, 4), dtype=np.uint8),
             bc=rng.integers(0, 256, (H, W, 3), dtype=np.uint8), parsing=PARSING[rng.integers(0, len(PARSING), (n, H, W))],
             teeth=rng.random((n, H, W)) < 0.15)
    a["torso"][..., 3] = rng.choice(np.array([0, 255, 1, 254, 128, 77, 200], dtype=np.uint8), (n, H, W))
    lms = rng.random((n, 68, 2)) * np.array([W - 1, H - 1])
    for i in range(n):                                  # inner-mouth extent (rows 60..67, column 1) differs per frame
        lms[i, 60:68, 1] = 8 + np.linspace(0, 1 + i, 8)
    a["lms"] = lms
    frames = []
    for i in range(n):
        c2w = np.eye(4)
        ang = 0.1 * (i - 4)
        c2w[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        c2w[:3, 3] = rng.standard_normal(3) * 0.05 + np.array([0, 0, 3.0])
        frames.append(c2w)
    a["c2w"] = np.array(frames)
    a["focal_len"] = np.float64(60.0)
    cols = ["frame", "AU01_r", "AU04_r", "AU05_r", "AU06_r", "AU07_r", "AU25_r", "AU45_r"]
    rows = np.round(rng.random((n + 1, len(cols))) * 3.0, 2)            # AU45 beyond 2: the clip matters
    rows[:, 0] = np.arange(n + 1)
    text = ",".join(cols) + "\n" + "".join(",".join(repr(float(v)) for v in r) + "\n" for r in rows)
    a["au_csv"] = np.frombuffer(text.encode(), dtype=np.uint8)
    a["aud_ds"] = rng.standard_normal((T_AUDIO, 16, 29)).astype(np.float32)
    a["drive"] = rng.standard_normal((T_AUDIO, 16, 29)).astype(np.float32)
    for k in ("a", "b"):                                                  # two sapiens folders: the latest (_b) is read
        a[f"normal_{k}"] = rng.standard_normal((len(TRAIN_IDS), H, W, 3)).astype(np.float32)
        a[f"depth_{k}"] = rng.random((len(TRAIN_IDS), H, W)).astype(np.float32)
    return a


def write_identity(root, a):
    """Lay the arrays out as files.  Images are written lossless (.png, the reader's ``extension`` parameter); bc.jpg
    holds PNG data under the name the reference opens (image libraries go by content)."""
    from PIL import Image
    ids = TRAIN_IDS + VAL_IDS
    for d in ("gt_imgs", "torso_imgs", "parsing", "teeth_mask", "ori_imgs", "sapiens/normal/sapiens_a",
              "sapiens/normal/sapiens_b", "sapiens/depth/sapiens_a", "sapiens/depth/sapiens_b"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for j, i in enumerate(ids):
        Image.fromarray(np.asarray(a["gt"][j]), "RGB").save(os.path.join(root, "gt_imgs", f"{i}.png"))
        Image.fromarray(np.asarray(a["torso"][j]), "RGBA").save(os.path.join(root, "torso_imgs", f"{i}.png"))
        Image.fromarray(np.asarray(a["parsing"][j]), "RGB").save(os.path.join(root, "parsing", f"{i}.png"))
        np.save(os.path.join(root, "teeth_mask", f"{i}.npy"), np.asarray(a["teeth"][j]).astype(bool))
        np.savetxt(os.path.join(root, "ori_imgs", f"{i}.lms"), np.asarray(a["lms"][j]))
    Image.fromarray(np.asarray(a["bc"]), "RGB").save(os.path.join(root, "bc.jpg"), format="PNG")
    for name, sel in (("train", TRAIN_IDS), ("val", VAL_IDS)):
        frames = [dict(img_id=int(i), transform_matrix=np.asarray(a["c2w"][ids.index(i)]).tolist()) for i in sel]
        with open(os.path.join(root, f"transforms_{name}.json"), "w") as f:
            json.dump(dict(focal_len=float(a["focal_len"]), frames=frames), f)
    with open(os.path.join(root, "au.csv"), "wb") as f:
        f.write(np.asarray(a["au_csv"]).tobytes())
    np.save(os.path.join(root, "aud_ds.npy"), np.asarray(a["aud_ds"]))
    np.save(os.path.join(root, "drive.npy"), np.asarray(a["drive"]))
    for k in ("a", "b"):
        for j, i in enumerate(TRAIN_IDS):
            np.save(os.path.join(root, "sapiens/normal", f"sapiens_{k}", f"{i}.npy"), np.asarray(a[f"normal_{k}"][j]))
            np.save(os.path.join(root, "sapiens/depth", f"sapiens_{k}", f"{i}.npy"), np.asarray(a[f"depth_{k}"][j]))
