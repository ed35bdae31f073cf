"""GPU: csrc/prepare.hip against the plain statements of instag_amd.prepare.  Everything is integer image work, so every
comparison is for exact equality on every byte."""
import os

import numpy as np
import pytest
import torch

from instag_amd import prepare as P
from tests import prepare_helpers as PH

pytestmark = pytest.mark.gpu
SHAPES = ((72, 40), (64, 33), (80, 130))      # the golden's size; odd width at the minimum height; nine 16-column strips
_CACHE = {}


def _case(shape):
    """Per shape, once: 9 scene frames + the 3 hand-built ones, and the statement's answers."""
    if shape not in _CACHE:
        H, W = shape
        ori, par = PH.scene(9, H, W, seed=H + W)
        s_ori, s_par, _ = PH.special_frames(H, W)
        bc, max_d2, arg = P.background_torch(ori[::2], par[::2])
        ori, par = np.concatenate([ori, s_ori]), np.concatenate([par, s_par])
        gt, torso = P.frames_torch(ori, par, bc)
        _CACHE[shape] = dict(ori=ori, par=par, bc=bc, max_d2=max_d2, arg=arg, gt=gt, torso=torso)
    return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_background(shape):
    c = _case(shape)
    bc, max_d2, arg = P.background(c["ori"][:9:2], c["par"][:9:2], "cuda")
    assert bc.dtype == torch.uint8 and max_d2.dtype == torch.int32 and arg.dtype == torch.int32
    assert torch.equal(max_d2.cpu(), c["max_d2"]) and torch.equal(arg.cpu(), c["arg"])
    assert torch.equal(bc.cpu(), c["bc"])
    known = c["max_d2"] > 25
    assert 0 < int(known.sum()) < known.numel() and len(torch.unique(c["arg"])) > 1
    assert torch.equal(P.extract_background(torch.from_numpy(c["ori"][:9]).cuda(), torch.from_numpy(c["par"][:9]).cuda(),
                                            every=2).cpu(), c["bc"])


def test_background_one_sample_and_a_repeated_sample():
    c = _case(SHAPES[0])
    ori, par = c["ori"][:9:2], c["par"][:9:2]
    for sel in ([3], [1, 0, 1, 0, 4]):                      # a repeated sample never wins over its first occurrence
        want = P.background_torch(ori[sel], par[sel])
        got = P.background(ori[sel], par[sel], "cuda")
        for g, w, name in zip(got, want, ("bc", "max_d2", "arg")):
            assert torch.equal(g.cpu(), w), (sel, name)
    assert set(torch.unique(got[2].cpu()).tolist()) <= {0, 1, 4}


def test_background_errors():
    c = _case(SHAPES[1])
    ori, par = c["ori"][:3].copy(), c["par"][:3].copy()
    par[2] = 255
    with pytest.raises(ValueError, match="sample 2 has no non-background pixel"):
        P.background(ori, par, "cuda")
    par[:] = 255
    par[:, ::4, ::4] = 0
    with pytest.raises(ValueError, match="no pixel"):
        P.background(ori, par, "cuda")
    with pytest.raises(ValueError, match="H >= 64"):
        P.gt_and_torso(ori[:, :63], par[:, :63], c["bc"][:63], device="cuda")


@pytest.mark.parametrize("shape", SHAPES)
def test_frames_into_prefilled_buffers(shape):
    c = _case(shape)
    H, W = shape
    N = len(c["ori"])
    gt = torch.full((N, H, W, 3), 0xA5, dtype=torch.uint8, device="cuda")
    torso = torch.full((N + 1, H, W, 4), 0xA5, dtype=torch.uint8, device="cuda")
    guard = torch.full((2, H * W * 4), 0xA5, dtype=torch.uint8, device="cuda")     # (neighbours in the allocator's block)
    P.frames_into(c["ori"], c["par"], c["bc"].cuda(), gt, torso[:N], batch=N)
    assert torch.equal(gt.cpu(), c["gt"]) and torch.equal(torso[:N].cpu(), c["torso"])
    assert bool((torso[N] == 0xA5).all()) and bool((guard == 0xA5).all())
    assert int((c["torso"][..., 3] == 255).sum()) > 0 and int((c["torso"][..., 3] == 0).sum()) > 0


def test_frames_batch_split():
    c = _case(SHAPES[0])
    ori, par = c["ori"][7:12], c["par"][7:12]               # two scene frames and the three hand-built ones
    gt, torso = P.gt_and_torso(ori, par, c["bc"], batch=2, device="cuda")
    assert torch.equal(gt.cpu(), c["gt"][7:12]) and torch.equal(torso.cpu(), c["torso"][7:12])


def test_prepare_identity_feeds_the_frame_store(tmp_path):
    from PIL import Image
    from instag_amd.frame_store import FrameStore, ingest_torch
    from tests.frame_store_helpers import cameras
    H, W = SHAPES[0]
    c = _case(SHAPES[0])
    ori, par = c["ori"][:9], c["par"][:9]
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "ori_imgs"))
    os.makedirs(os.path.join(root, "parsing"))
    for i in range(9):                                      # (stems 2 and 10: a sort by name would swap them)
        stem = i if i < 8 else 10
        Image.fromarray(ori[i], "RGB").save(os.path.join(root, "ori_imgs", f"{stem}.jpg"), quality=95)
        Image.fromarray(par[i], "RGB").save(os.path.join(root, "parsing", f"{stem}.png"))
    dec = np.stack([np.array(Image.open(os.path.join(root, "ori_imgs", f"{s}.jpg")).convert("RGB"))
                    for s in list(range(8)) + [10]])
    bc, gt, torso = P.prepare_identity(root, "cuda", every=2, write=True)
    w_bc = P.background_torch(dec[::2], par[::2])[0]
    w_gt, w_torso = P.frames_torch(dec, par, w_bc)
    assert torch.equal(bc.cpu(), w_bc) and torch.equal(gt.cpu(), w_gt) and torch.equal(torso.cpu(), w_torso)
    teeth = np.zeros((9, H, W), dtype=np.uint8)
    store = FrameStore("cuda")
    store.append(gt, torso, bc, torch.from_numpy(par).cuda(), teeth, cameras(9, H, W), torch.zeros(9, 6),
                 torch.zeros(9, 4, dtype=torch.int32), [0] * 9)
    want = ingest_torch(w_gt, w_torso, w_bc, torch.from_numpy(par), torch.from_numpy(teeth))
    for g, w in zip(store.planes(), want):
        assert torch.equal(g.cpu(), w)
    # the written files: the torso PNGs are lossless, the JPEGs decode to the image's size
    back = np.array(Image.open(os.path.join(root, "torso_imgs", "10.png")).convert("RGBA"))
    assert np.array_equal(back, w_torso[8].numpy())
    assert Image.open(os.path.join(root, "bc.jpg")).size == (W, H)
    assert sorted(os.listdir(os.path.join(root, "gt_imgs"))) == sorted(f"{s}.jpg" for s in list(range(8)) + [10])


def test_symbols():
    from instag_amd import _lib
    lib = _lib.lib()
    for n in ("instag_prep_background_workspace_bytes", "instag_prep_background", "instag_prep_frames"):
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n)
