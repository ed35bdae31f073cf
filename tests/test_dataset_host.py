"""CPU: instag_amd.dataset against golden G10 (the reference's readCamerasFromTransforms on a tiny identity directory,
tests/golden/make_golden_dataset.py) and FrameSampler against a transcription of the reference's sampling loops."""
import json
import os
import random

import numpy as np
import pytest
import torch

from instag_amd import dataset as DS
from instag_amd import frame_store as FS
from tests import dataset_helpers as D


@pytest.fixture(scope="module")
def g10(golden_dir):
    g = np.load(f"{golden_dir}/g10_dataset.npz")
    return g, {k[3:]: g[k] for k in g.files if k.startswith("in.")}


def _rows(ids):
    order = D.TRAIN_IDS + D.VAL_IDS
    return [order.index(int(i)) for i in ids]


@pytest.mark.parametrize("tag,split,n_views,audio", D.CALLS)
def test_array_level_parts_reproduce_the_reference(g10, tmp_path, tag, split, n_views, audio):
    """No image library involved: the table from the parsed transforms, au.csv and the landmarks; the composite and
    the masks from the recorded input arrays through ingest_torch; the audio windows through audio_window."""
    g, a = g10
    with open(tmp_path / "au.csv", "wb") as f:
        f.write(a["au_csv"].tobytes())
    au = DS.read_au_csv(tmp_path / "au.csv")
    order = D.TRAIN_IDS + D.VAL_IDS
    sel = D.TRAIN_IDS if split == "train" else D.VAL_IDS
    contents = dict(focal_len=float(a["focal_len"]),
                    frames=[dict(img_id=i, transform_matrix=a["c2w"][order.index(i)].tolist()) for i in sel])
    lms = {i: a["lms"][j] for j, i in enumerate(order)}
    feats = a["drive"] if audio else a["aud_ds"]
    t = DS.identity_table(contents, au, lms, feats.shape[0], split, audio_file=audio, n_views=n_views, size=(D.W, D.H))
    for k in ("img_id", "blink", "au25", "au_exp", "lips_rect", "lhalf_rect", "mouth_bound", "R", "T"):
        assert np.array_equal(t[k], g[f"{tag}.{k}"]), (tag, k)
    assert t["au_exp"].dtype == np.float32 and len(t["img_id"]) == {"train": 5, "val": 2, "train4": 4, "val_audio": 10}[tag]
    assert np.all(g[f"{tag}.FovX"] == t["FovX"]) and np.all(g[f"{tag}.FovY"] == t["FovY"])
    rows = _rows(t["img_id"])
    rgb, bg, mask, counts = FS.ingest_torch(*(torch.from_numpy(np.ascontiguousarray(x)) for x in (
        a["gt"][rows], a["torso"][rows], a["bc"], a["parsing"][rows], a["teeth"][rows].astype(np.uint8))))
    assert np.array_equal(rgb.numpy(), g[f"{tag}.image"]) and np.array_equal(bg.numpy(), g[f"{tag}.background"])
    for bit, k in enumerate(("face_mask", "hair_mask", "mouth_mask")):
        assert np.array_equal(((mask.numpy() >> bit) & 1).astype(bool), g[f"{tag}.{k}"]), (tag, k)
        assert np.array_equal(counts[:, bit].numpy(), g[f"{tag}.{k}"].reshape(len(rows), -1).sum(1))
    table = torch.from_numpy(feats).float().permute(0, 2, 1)
    auds = torch.stack([FS.audio_window(table, int(i)) for i in t["audio_index"]])
    assert np.array_equal(auds.numpy(), g[f"{tag}.auds"]) and tuple(auds.shape[1:]) == (8, 29, 16)


@pytest.mark.parametrize("tag,split,n_views,audio", D.CALLS)
def test_read_identity_reproduces_the_reference(g10, tmp_path, tag, split, n_views, audio):
    pytest.importorskip("PIL")
    g, a = g10
    root = str(tmp_path)
    D.write_identity(root, a)
    kw = dict(audio_file=os.path.join(root, audio) if audio else "", n_views=n_views, extension=".png")
    d = DS.read_identity(root, split, **kw)
    rows = _rows(d["meta"]["img_id"])
    for k in ("gt", "torso", "parsing"):
        assert np.array_equal(d[k], a[k][rows]), k
    assert np.array_equal(d["bc"], a["bc"]) and np.array_equal(d["teeth"].astype(bool), a["teeth"][rows])
    for k in ("img_id", "blink", "au25", "mouth_bound", "R", "T"):
        assert np.array_equal(d["meta"][k], g[f"{tag}.{k}"]), k
    assert np.all(g[f"{tag}.FovX"] == d["meta"]["FovX"]) and np.all(g[f"{tag}.FovY"] == d["meta"]["FovY"])
    assert np.array_equal(d["lhalf_rect"], g[f"{tag}.lhalf_rect"])
    assert ("normal" in d) == (tag == "train4")
    # ... and through a store on the CPU device: what a step is fed == what the reference would upload
    store, meta = DS.open_identity(root, split, "cpu", batch=3, **kw)
    n = len(store)
    assert n == len(g[f"{tag}.img_id"]) and meta["blink"].shape == (n,)
    assert (store.FoVx, store.FoVy) == (d["meta"]["FovX"], d["meta"]["FovY"])
    assert np.array_equal(store.counts[:, 2].numpy(), g[f"{tag}.mouth_mask"].reshape(n, -1).sum(1))
    for i in range(n):
        u = store.unpack_torch(i)
        assert torch.equal(u["original_image"], torch.from_numpy(g[f"{tag}.image"][i]).permute(2, 0, 1) / 255.0)
        assert torch.equal(u["background"], torch.from_numpy(g[f"{tag}.background"][i]).permute(2, 0, 1) / 255.0)
        for k in ("face_mask", "hair_mask", "mouth_mask", "auds", "au_exp"):
            assert np.array_equal(u[k].numpy(), g[f"{tag}.{k}"][i]), (k, i)
        assert u["lips_rect"].tolist() == g[f"{tag}.lips_rect"][i].tolist()
        R, Tr = g[f"{tag}.R"][i], g[f"{tag}.T"][i]
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = R.T, Tr
        assert np.allclose(u["world_view_transform"].numpy(), np.float32(w2c).T, atol=1e-6)       # cameras.py:55
        if tag == "train4":
            assert np.array_equal(u["normal"].numpy(), g[f"{tag}.normal"][i])
            assert np.array_equal(u["depth"].numpy(), g[f"{tag}.depth"][i])
            assert np.array_equal(u["normal"].numpy(), a["normal_b"][rows[i]].transpose(2, 0, 1))  # the latest folder
    assert DS.read_identity(root, "train", n_views=4, extension=".png", preload_priors=False).get("normal") is None


def test_dataset_module_does_not_import_an_image_library_at_import_time():
    import subprocess
    import sys
    code = "import sys; import instag_amd.dataset; sys.exit(1 if any(m == 'PIL' or m.startswith('PIL.') for m in sys.modules) else 0)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


# ---- FrameSampler ----------------------------------------------------------------------------------------------------
def _table(n=40):
    """Mouth openings at both extremes (nothing in between: late in the warm phase no frame lies in the window), blinks
    below 0.3 (late in the blink phase none does either); AU25 spread evenly, a few frames with a tiny mouth mask."""
    rng = np.random.default_rng(4)
    opening = np.where(np.arange(n) % 4 == 3, 30 - (np.arange(n) % 3), np.arange(n) % 2)
    mouth_bound = np.stack([np.full(n, opening.min()), np.full(n, opening.max()), opening], axis=1)
    blink = rng.random(n) * 0.3
    au = rng.permutation(np.linspace(0.0, 2.0, n))
    au25 = np.stack([au] + [np.full(n, np.percentile(au, q)) for q in (25, 50, 75)] + [np.full(n, au.max())], axis=1)
    counts = np.zeros((n, 3), dtype=np.int64)
    counts[:, 2] = np.where(np.arange(n) % 7 == 2, 5, 400)
    return dict(blink=blink, au25=au25, mouth_bound=mouth_bound), counts


def _face_loop(cams, rng, iterations, warm_step=3000, select_interval=10):
    """train_face.py:122-301 (prints dropped)."""
    randint = rng.randint
    mouth_select_iter = iterations
    mouth_step = 1 / max(mouth_select_iter, 1)
    viewpoint_stack, out, fallbacks = None, [], 0
    for iteration in range(1, iterations + 1):
        if not viewpoint_stack:
            viewpoint_stack = cams.copy()
        viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))
        mouth_global_lb = viewpoint_cam['mouth_bound'][0]
        mouth_global_ub = viewpoint_cam['mouth_bound'][1]
        mouth_global_lb += (mouth_global_ub - mouth_global_lb) * 0.2
        mouth_window = (mouth_global_ub - mouth_global_lb) * 0.5
        mouth_lb = mouth_global_lb + mouth_step * iteration * (mouth_global_ub - mouth_global_lb)
        mouth_ub = mouth_lb + mouth_window
        mouth_lb = mouth_lb - mouth_window
        au_global_lb = 0
        au_global_ub = 1
        au_window = 0.4
        au_lb = au_global_lb + mouth_step * iteration * (au_global_ub - au_global_lb)
        au_ub = au_lb + au_window
        au_lb = au_lb - au_window * 1.5
        for key, lb, ub, on in (('mouth', mouth_lb, mouth_ub, iteration < warm_step and iteration < mouth_select_iter),
                                ('blink', au_lb, au_ub, warm_step < iteration < mouth_select_iter)):
            val = (lambda c: c['mouth_bound'][2]) if key == 'mouth' else (lambda c: c['blink'])
            if on:
                if iteration % select_interval == 0:
                    max_attempts = 100
                    attempts = 0
                    while (val(viewpoint_cam) < lb or val(viewpoint_cam) > ub) and attempts < max_attempts:
                        if not viewpoint_stack:
                            viewpoint_stack = cams.copy()
                        viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))
                        attempts += 1
                    if attempts >= max_attempts:
                        fallbacks += 1
                        best_cam = None
                        min_distance = float('inf')
                        for cam in cams:
                            v = val(cam)
                            if v < lb:
                                distance = lb - v
                                if distance < min_distance:
                                    min_distance = distance
                                    best_cam = cam
                            elif v > ub:
                                distance = v - ub
                                if distance < min_distance:
                                    min_distance = distance
                                    best_cam = cam
                            else:
                                best_cam = cam
                                break
                        if best_cam is not None:
                            viewpoint_cam = best_cam
        out.append(viewpoint_cam['index'])
    return out, fallbacks


def _mouth_loop(cams, rng, iterations, warm_step=3000, select_interval=5, give_up=100000):
    """train_mouth.py:119-148; ``give_up`` only guards the test against a table on which the loops would not end."""
    randint = rng.randint
    mouth_select_iter = iterations
    mouth_step = 1 / mouth_select_iter
    viewpoint_stack, out, longest = None, [], 0
    for iteration in range(1, iterations + 1):
        draws = 0
        if not viewpoint_stack:
            viewpoint_stack = cams.copy()
        viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))
        au_global_lb = viewpoint_cam['au25'][1]
        au_global_ub = viewpoint_cam['au25'][3]
        au_ub = au_global_ub
        au_lb = au_ub - mouth_step * iteration * (au_global_ub - au_global_lb)
        if iteration < warm_step:
            while viewpoint_cam['au25'][0] < au_global_ub:
                if not viewpoint_stack:
                    viewpoint_stack = cams.copy()
                viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))
                draws += 1
                assert draws < give_up
            longest, draws = max(longest, draws), 0
        if warm_step < iteration < mouth_select_iter:
            if iteration % select_interval == 0:
                while viewpoint_cam['au25'][0] < au_lb or viewpoint_cam['au25'][0] > au_ub:
                    if not viewpoint_stack:
                        viewpoint_stack = cams.copy()
                    viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))
                    draws += 1
                    assert draws < give_up
                longest, draws = max(longest, draws), 0
            while viewpoint_cam['mouth_pixels'] < 20:
                if not viewpoint_stack:
                    viewpoint_stack = cams.copy()
                viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))
                draws += 1
                assert draws < give_up
            longest = max(longest, draws)
        out.append(viewpoint_cam['index'])
    return out, longest


def _cams(meta, counts):
    return [dict(index=i, blink=float(meta["blink"][i]), au25=meta["au25"][i].tolist(),
                 mouth_bound=meta["mouth_bound"][i].tolist(), mouth_pixels=int(counts[i, 2]))
            for i in range(len(meta["blink"]))]


def test_face_sampler_is_the_reference_loop_over_a_full_schedule():
    meta, counts = _table()
    want, fallbacks = _face_loop(_cams(meta, counts), random.Random(17), 10000)
    s = DS.FrameSampler(meta, "face", seed=17, iterations=10000)
    got = [s.next(it) for it in range(1, 10001)]
    assert got == want
    assert fallbacks >= 1 and s.capped == fallbacks                     # the nearest-frame fallback was reached
    assert len(set(got)) == 40


def test_mouth_sampler_is_the_reference_loop_over_a_full_schedule():
    meta, counts = _table()
    want, longest = _mouth_loop(_cams(meta, counts), random.Random(23), 10000)
    s = DS.FrameSampler(meta, "mouth", seed=23, counts=torch.from_numpy(counts), iterations=10000)
    got = [s.next(it) for it in range(1, 10001)]
    assert got == want
    assert s.capped == 0 and longest < 100          # the reference's loops ended by themselves: the cap never acted
    small = {i for i in range(40) if counts[i, 2] < 20}
    assert small and not (small & set(got[3000:9999]))
    with pytest.raises(ValueError):
        DS.FrameSampler(meta, "mouth")


def test_mouth_sampler_is_bounded_where_the_reference_would_not_end():
    """The one deviation: no frame has 20 mouth pixels -> 100 attempts, then the nearest (most pixels) frame."""
    meta, counts = _table()
    counts[:, 2] = np.arange(40) % 19
    s = DS.FrameSampler(meta, "mouth", seed=1, counts=counts, iterations=10000)
    assert s.next(3001) == 18 and s.capped == 1


def test_fuse_sampler_is_the_plain_pop():
    meta, _ = _table()
    rng, stack, want = random.Random(5), [], []
    for _ in range(100):
        if not stack:
            stack = list(range(40))
        want.append(stack.pop(rng.randint(0, len(stack) - 1)))
    s = DS.FrameSampler(meta, "fuse", seed=5)
    assert [s.next(i + 1) for i in range(100)] == want and sorted(want[:40]) == list(range(40))
