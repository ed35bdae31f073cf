"""Shared inputs of the frame-store tests (host and GPU): the exhaustive composite triples, seeded raw frames whose
parsing images hit every mask rule and its near misses, and a store built from them."""
import numpy as np
import torch

# the three colours the reference's rules key on, and what must NOT match: blue 254, mouth grey off by one, almost
# black, blue with a trace of red; plus a colour that is none of them
PALETTE = np.array([(0, 0, 255), (0, 0, 0), (100, 100, 100), (255, 255, 255),
                    (0, 0, 254), (100, 100, 99), (0, 0, 1), (1, 0, 255), (255, 0, 0), (0, 1, 255), (99, 100, 100)],
                   dtype=np.uint8)
SHAPES = ((5, 7), (6, 6), (16, 16), (37, 53))       # H*W odd, H*W % 4 == 0 (36, 256), 1961 = neither


def composite_numpy(torso, bc):
    """dataset_readers.py:232-235, literally (torso uint8 RGBA [...,4], bc uint8 [...,3])."""
    torso_img = np.asarray(torso) * 1.0
    bg_img = np.asarray(bc)
    bg = torso_img[..., :3] * torso_img[..., 3:] / 255.0 + bg_img * (1 - torso_img[..., 3:] / 255.0)
    return bg.astype(np.uint8)


def triples(rows=slice(0, 4096)):
    """All 256^3 (torso, alpha, bc) triples as a 4096 x 4096 image (or some of its rows), each value in every channel:
    pixel (y, x): torso = y >> 4, alpha = (y & 15) << 4 | x >> 8, bc = x & 255."""
    y = np.arange(4096, dtype=np.int64)[rows, None]
    x = np.arange(4096, dtype=np.int64)[None, :]
    t = np.broadcast_to(y >> 4, (y.shape[0], 4096)).astype(np.uint8)
    a = (((y & 15) << 4) | (x >> 8)).astype(np.uint8)
    b = np.broadcast_to(x & 255, (y.shape[0], 4096)).astype(np.uint8)
    torso = np.stack([t, t, t, a], axis=-1)
    bc = np.stack([b, b, b], axis=-1)
    return torso, bc


def raw_frames(F, H, W, seed, priors=False, empty_mouth_frame=1):
    """Decoded files of F frames: dict of uint8 arrays (+ fp32 priors).  Teeth overlap face (blue) and mouth (grey)
    pixels as well as others; frame ``empty_mouth_frame`` has neither teeth nor mouth-grey pixels."""
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    torso = rng.integers(0, 256, (F, H, W, 4), dtype=np.uint8)
    torso[..., 3] = rng.choice(np.array([0, 255, 1, 254, 128, 77], dtype=np.uint8), (F, H, W))
    bc = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    idx = rng.integers(0, len(PALETTE), (F, H, W))
    idx.reshape(F, -1)[:, :len(PALETTE)] = np.arange(min(len(PALETTE), H * W))    # every colour in every frame
    teeth = (rng.random((F, H, W)) < 0.3)
    teeth.reshape(F, -1)[:, :len(PALETTE)] = (np.arange(F)[:, None] + np.arange(len(PALETTE))[None]) % 2 == 0
    if 0 <= empty_mouth_frame < F:
        idx[empty_mouth_frame][idx[empty_mouth_frame] == 2] = 3
        teeth[empty_mouth_frame] = False
    out = dict(gt=gt, torso=torso, bc=bc, parsing=PALETTE[idx], teeth=teeth.astype(np.uint8))
    if priors:
        out["normal"] = rng.standard_normal((F, 3, H, W)).astype(np.float32)
        out["depth"] = rng.random((F, H, W)).astype(np.float32)
    return out


def masks_numpy(parsing, teeth):
    """dataset_readers.py:246-249, literally (teeth as the bool array np.load returns)."""
    mask = np.asarray(parsing) * 1.0
    teeth_mask = np.asarray(teeth).astype(bool)
    face = (mask[..., 2] > 254) * (mask[..., 0] == 0) * (mask[..., 1] == 0) ^ teeth_mask
    hair = (mask[..., 0] < 1) * (mask[..., 1] < 1) * (mask[..., 2] < 1)
    mouth = (mask[..., 0] == 100) * (mask[..., 1] == 100) * (mask[..., 2] == 100) + teeth_mask
    return face, hair, mouth


def cameras(F, H, W):
    from instag_amd.scene_synth import camera_from_c2w
    import json
    import os
    from instag_amd import scene_synth
    with open(os.path.join(os.path.dirname(scene_synth.__file__), "data", "toy_cameras.json")) as f:
        d = json.load(f)
    return [camera_from_c2w(d["frames"][i % len(d["frames"])]["transform_matrix"], d["focal_len"] * W / 512.0, W, H)
            for i in range(F)]


def audio_table(T, C, L, seed):
    return torch.randn(T, C, L, generator=torch.Generator().manual_seed(seed))


def build_store(device, F, H, W, seed, audio_index, audio, priors=False, split=None):
    """(store, raw) with au_exp / lips_rect drawn from the seed; ``split``: appended as two batches [:split], [split:]."""
    from instag_amd.frame_store import FrameStore
    raw = raw_frames(F, H, W, seed, priors=priors)
    g = torch.Generator().manual_seed(seed)
    raw["au_exp"] = torch.rand(F, 6, generator=g)
    raw["lips_rect"] = torch.randint(0, max(H, W), (F, 4), generator=g, dtype=torch.int32)
    raw["cameras"] = cameras(F, H, W)
    store = FrameStore(device)
    for part in ((slice(0, F),) if split is None else (slice(0, split), slice(split, F))):
        store.append(raw["gt"][part], raw["torso"][part], raw["bc"], raw["parsing"][part], raw["teeth"][part],
                     raw["cameras"][part], raw["au_exp"][part], raw["lips_rect"][part], list(audio_index)[part],
                     normal=raw["normal"][part] if priors else None, depth=raw["depth"][part] if priors else None)
    store.set_audio(audio)
    return store, raw


def synthetic_store(device, F, size, T=12, audio_extractor="deepspeech"):
    """A store whose frames look like scene_synth.synthetic_frame (a head disc, a hair cap, a mouth disc with teeth
    in it, a sane lips_rect), quantised to the 8-bit files a processed identity holds."""
    from instag_amd.frame_store import FrameStore
    from instag_amd.scene_synth import synthetic_frame, toy_cameras
    raw = {k: [] for k in ("gt", "torso", "parsing", "teeth", "au_exp", "lips_rect")}
    rng = np.random.default_rng(size)
    for i in range(F):
        s = synthetic_frame(size, i)
        raw["gt"].append((s["gt_image"].permute(1, 2, 0) * 255).to(torch.uint8).numpy())
        par = np.full((size, size, 3), 255, dtype=np.uint8)
        par[s["face_mask"].numpy()] = (0, 0, 255)
        par[s["hair_mask"].numpy()] = (0, 0, 0)
        par[s["mouth_mask"].numpy()] = (100, 100, 100)
        raw["parsing"].append(par)
        raw["teeth"].append((s["mouth_mask"].numpy() & (rng.random((size, size)) < 0.4)).astype(np.uint8))
        raw["torso"].append(rng.integers(0, 256, (size, size, 4), dtype=np.uint8))
        raw["au_exp"].append(s["au_exp"])
        raw["lips_rect"].append(s["lips_rect"])
    raw = {k: (torch.stack(v) if torch.is_tensor(v[0]) else np.stack(v)) for k, v in raw.items()}
    raw["bc"] = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
    raw["cameras"] = toy_cameras(size, F)
    C, L = (1, 512) if audio_extractor == "ave" else (29, 16)
    store = FrameStore(device)
    store.append(raw["gt"], raw["torso"], raw["bc"], raw["parsing"], raw["teeth"], raw["cameras"], raw["au_exp"],
                 raw["lips_rect"], [(3 * i + 1) % T for i in range(F)])
    store.set_audio(audio_table(T, C, L, 5))
    return store
