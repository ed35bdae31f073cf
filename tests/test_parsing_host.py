"""CPU tests of the face-parsing statement (instag_amd/parsing.py) against golden G14 -- the reference's own BiSeNet(19)
in fp64 under the seeded rule of tests/parsing_helpers.py -- and of the weights' layout, the colour table, the nearest
resize and the directory entry point."""
import json
import os

import numpy as np
import pytest
import torch

from tests import parsing_helpers as H


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(f"{golden_dir}/g14_parsing.npz")


@pytest.fixture(scope="module")
def g14_weights():
    return H.weights()


def test_logits_and_labels_match_g14(g14, g14_weights):
    from instag_amd import parsing as P
    frame = torch.from_numpy(g14["frame"])[None]
    assert torch.equal(frame, H.seeded_frames(1, H.G14_H, H.G14_W))
    taps = []
    with torch.no_grad():
        got = P.bisenet_torch(g14_weights, P.normalise(frame, torch.float64), taps)
    want = torch.from_numpy(g14["logits8"])[None]
    assert got.dtype == torch.float64 and tuple(got.shape) == (1, 19, 8, 12)
    err = float((got - want).abs().max()) / float(want.abs().max())
    print(f"logits at 1/8: {err:.3e} of the largest entry")
    assert err <= 1e-9
    full = P.upsample_torch(got, H.G14_H, H.G14_W)
    assert float((full[0] - torch.from_numpy(g14["full"])).abs().max()) <= 1e-9 * float(want.abs().max())
    labels = P.labels_torch(got, H.G14_H, H.G14_W)
    assert labels.dtype == torch.uint8 and np.array_equal(labels[0].numpy(), g14["labels"])
    assert len(np.unique(g14["labels"])) >= 5
    assert np.allclose(H.liveness(taps), g14["positive"], atol=1e-12)
    assert all(0.2 <= p <= 0.8 for p in g14["positive"])


def test_state_dict_layout_matches_g14(g14):
    layout = json.loads(bytes(g14["layout"]).decode())
    sd = H.state_dict()
    assert sorted((k, list(v.shape)) for k, v in sd.items()) == [(k, s) for k, s in layout]
    assert len(sd) == 191
    assert sum(v.numel() for v in sd.values()) == 13313119


def test_aux_heads_ignored_and_missing_key_named():
    from instag_amd.parsing import BiSeNetWeights
    sd = H.state_dict()
    full = BiSeNetWeights.from_state_dict(sd)
    lean = {k: v for k, v in sd.items()
            if not k.startswith(("conv_out16.", "conv_out32.")) and not k.endswith("num_batches_tracked")}
    assert len(lean) < len(sd)
    trimmed = BiSeNetWeights.from_state_dict(lean)
    for a, b in zip(full.layers, trimmed.layers):
        assert a.keys() == b.keys() and all(torch.equal(a[f], b[f]) for f in a)
    garbled = dict(sd)
    garbled["conv_out16.conv_out.weight"] = torch.zeros(1)       # never read, so never checked
    BiSeNetWeights.from_state_dict(garbled)
    for key in ("cp.resnet.layer2.0.downsample.0.weight", "cp.arm16.conv_atten.weight", "ffm.conv1.weight",
                "conv_out.conv_out.weight", "cp.resnet.bn1.running_var"):
        broken = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            BiSeNetWeights.from_state_dict(broken)


def test_colour_table():
    from instag_amd import parsing as P
    from instag_amd import prepare
    labels = torch.arange(19, dtype=torch.uint8).view(1, 1, 19)
    col = P.colour_map_torch(labels)[0, 0].numpy()
    assert col.dtype == np.uint8 and col.shape == (19, 3)
    want = {0: prepare.BACKGROUND, 1: prepare.HEAD, 14: prepare.NECK, 16: prepare.TORSO, 11: (100, 100, 100),
            17: (0, 0, 0), 18: prepare.HEAD}
    for c, rgb in want.items():
        assert tuple(col[c]) == rgb, c
    for c in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13):
        assert tuple(col[c]) == prepare.HEAD, c
    assert tuple(col[15]) == prepare.NECK


def test_nearest_resize_rule(g14):
    from instag_amd import parsing as P
    labels = torch.from_numpy(g14["labels"])[None]
    got = P.colour_map_torch(labels, 50, 70)[0].numpy()
    ys, xs = H.numpy_resize_index(50, 64), H.numpy_resize_index(70, 96)
    assert ys[0] == 0 and ys[-1] == 62 and xs[-1] == 94 and len(set(ys)) == 50
    want = P.COLOURS[g14["labels"][ys[:, None], xs[None, :]]]
    assert got.shape == (50, 70, 3) and np.array_equal(got, want)
    # enlarging repeats pixels; the same size is the identity
    up = P.colour_map_torch(labels, 100, 96)[0].numpy()
    assert np.array_equal(up, P.COLOURS[g14["labels"][H.numpy_resize_index(100, 64)]])
    assert np.array_equal(P.colour_map_torch(labels)[0].numpy(), P.COLOURS[g14["labels"]])


def test_parse_identity_and_prepare_on_the_cpu(tmp_path):
    from PIL import Image
    from instag_amd import parsing as P
    from instag_amd import prepare
    weights = H.weights_with_background()
    os.makedirs(tmp_path / "ori_imgs")
    frames = H.seeded_frames(2, 80, 72, seed=5).numpy()
    for i in range(2):
        Image.fromarray(frames[i], "RGB").save(tmp_path / "ori_imgs" / f"{i}.jpg", quality=95)
    par = P.parse_identity(str(tmp_path), weights, device="cpu", batch=2)
    assert par.dtype == torch.uint8 and tuple(par.shape) == (2, 80, 72, 3) and par.device.type == "cpu"
    for i in range(2):
        img = Image.open(tmp_path / "parsing" / f"{i}.png")
        assert img.size == (72, 80) and img.mode == "RGB"
        assert np.array_equal(np.array(img), par[i].numpy())
    # what the reference does with a frame that is not 512 x 512 (test.py:94-106)
    resized = np.stack([np.array(Image.open(tmp_path / "ori_imgs" / f"{i}.jpg").resize((512, 512), Image.BILINEAR)
                                 .convert("RGB")) for i in range(2)])
    assert torch.equal(par, P.parse_torch(weights, torch.from_numpy(resized), out_size=(80, 72)))
    colours = {tuple(c) for c in par.reshape(-1, 3).tolist()}
    assert colours <= {tuple(c) for c in P.COLOURS.tolist()} and len(colours) >= 3
    assert prepare.BACKGROUND in colours and len(colours - {prepare.BACKGROUND}) >= 1
    from_files = prepare.prepare_identity(str(tmp_path), "cpu", every=1, write=False)
    from_tensor = prepare.prepare_identity(str(tmp_path), "cpu", every=1, write=False, parsing=par)
    from_array = prepare.prepare_identity(str(tmp_path), "cpu", every=1, write=False, parsing=par.numpy())
    for a, b, c in zip(from_files, from_tensor, from_array):
        assert torch.equal(a, b) and torch.equal(a, c)
    with pytest.raises(ValueError, match="parsing"):
        prepare.prepare_identity(str(tmp_path), "cpu", write=False, parsing=par[:1])
