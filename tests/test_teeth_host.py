"""CPU tests of the teeth-segmentation statement (instag_amd/teeth.py) against golden G15 -- the reference's own
ResNetV1c-50, FPN and FPNHead in fp64 under the seeded rule of tests/teeth_helpers.py -- and of the weights' layout, the
BatchNorm fold, the directory entry point and the library's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import teeth_helpers as H


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(f"{golden_dir}/g15_teeth.npz")


@pytest.fixture(scope="module")
def g15_weights():
    return H.weights()


def test_logits_and_labels_match_g15(g15, g15_weights):
    from instag_amd import teeth as T
    frame = torch.from_numpy(g15["frame"])[None]
    assert torch.equal(frame, H.seeded_frames(1, H.G15_H, H.G15_W))
    taps = []
    with torch.no_grad():
        got = T.fpn_torch(g15_weights, T.normalise(frame, torch.float64), taps)
    want = torch.from_numpy(g15["logits4"])[None]
    assert got.dtype == torch.float64 and tuple(got.shape) == (1, 8, 16, 24)
    err = float((got - want).abs().max()) / float(want.abs().max())
    print(f"logits at 1/4: {err:.3e} of the largest entry")
    assert err <= 1e-9
    full = T.upsample_torch(got, H.G15_H, H.G15_W)
    assert float((full[0] - torch.from_numpy(g15["full"])).abs().max()) <= 1e-9 * float(want.abs().max())
    labels = T.labels_torch(got, H.G15_H, H.G15_W)
    assert labels.dtype == torch.uint8 and np.array_equal(labels[0].numpy(), g15["labels"])
    assert len(np.unique(g15["labels"])) >= 5
    assert 0.002 <= float((g15["labels"] == T.TEETH).mean()) <= 0.5
    assert len(taps) == 30 and np.allclose(H.liveness(taps), g15["positive"], atol=1e-12)
    assert all(0.2 <= p <= 0.8 for p in g15["positive"])


def test_state_dict_layout_matches_g15(g15):
    from instag_amd import teeth as T
    layout = json.loads(bytes(g15["layout"]).decode())
    sd = H.state_dict()
    assert sorted((k, list(v.shape)) for k, v in sd.items()) == [(k, s) for k, s in layout]
    assert len(T.LAYERS) == 71 == sum(1 for v in sd.values() if v.dim() == 4)
    learnt = sum(v.numel() for k, v in sd.items() if v.dim() and not k.endswith(("running_mean", "running_var")))
    assert 28.4e6 < learnt < 28.7e6
    assert T.FPNWeights.random(H.SEED).classes == 8


def test_checkpoint_wrapper_and_bare_state_dict_load():
    from instag_amd.teeth import FPNWeights
    sd = H.state_dict()
    bare = FPNWeights.from_state_dict(sd)
    wrapped = FPNWeights.from_state_dict({"meta": {"CLASSES": ("background",)}, "state_dict": sd})
    lean = FPNWeights.from_state_dict({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")})
    for other in (wrapped, lean):
        for a, b in zip(bare.layers, other.layers):
            assert a.keys() == b.keys() and all(torch.equal(a[f], b[f]) for f in a)


def test_load_reads_a_checkpoint_file(tmp_path):
    from instag_amd.teeth import FPNWeights
    sd = H.state_dict()
    torch.save({"meta": {}, "state_dict": sd}, tmp_path / "ckpt.pth")
    got = FPNWeights.load(str(tmp_path / "ckpt.pth")).state_dict()
    assert got.keys() == sd.keys() and all(torch.equal(got[k], sd[k]) for k in sd)


def test_missing_key_wrong_shape_and_class_count_are_named():
    from instag_amd.teeth import FPNWeights
    sd = H.state_dict()
    for key in ("backbone.stem.3.weight", "backbone.layer3.0.downsample.0.weight", "backbone.layer4.2.bn3.running_var",
                "neck.lateral_convs.2.conv.bias", "neck.fpn_convs.0.conv.weight",
                "decode_head.scale_heads.3.4.bn.weight", "decode_head.conv_seg.bias"):
        broken = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            FPNWeights.from_state_dict(broken)
    bad = dict(sd)
    bad["backbone.layer2.1.conv2.weight"] = torch.zeros(128, 128, 1, 1)
    with pytest.raises(ValueError, match=r"backbone\.layer2\.1\.conv2 weight has shape \(128, 128, 1, 1\)"):
        FPNWeights.from_state_dict(bad)
    bad = dict(sd)
    bad["neck.lateral_convs.1.conv.bias"] = torch.zeros(255)
    with pytest.raises(ValueError, match=r"neck\.lateral_convs\.1\.conv bias"):
        FPNWeights.from_state_dict(bad)
    for classes in (7, 33):
        bad = dict(sd)
        bad["decode_head.conv_seg.weight"] = torch.zeros(classes, 128, 1, 1)
        bad["decode_head.conv_seg.bias"] = torch.zeros(classes)
        with pytest.raises(ValueError, match="8 <= C <= 32"):
            FPNWeights.from_state_dict(bad)
    nine = dict(sd)
    nine["decode_head.conv_seg.weight"] = torch.zeros(9, 128, 1, 1)
    nine["decode_head.conv_seg.bias"] = torch.zeros(9)
    assert FPNWeights.from_state_dict(nine).classes == 9


def test_folded_against_explicit_batch_norm(g15_weights):
    from instag_amd import teeth as T
    g = torch.Generator().manual_seed(1)
    folded = g15_weights.folded(torch.float64)
    p = g15_weights.to(dtype=torch.float64)
    for name in ("backbone.stem.0", "backbone.layer2.0.conv2", "backbone.layer3.0.downsample.0",
                 "decode_head.scale_heads.2.2.conv", "neck.lateral_convs.1.conv", "decode_head.conv_seg"):
        l = T.INDEX[name]
        _, bn, bias, cin, _, k, stride = T.LAYERS[l]
        x = torch.randn(2, cin, 9, 7, generator=g, dtype=torch.float64)
        lay = p[name]
        want = F.conv2d(x, lay["weight"], lay.get("bias"), stride=stride, padding=k // 2)
        if bn:
            want = F.batch_norm(want, lay["mean"], lay["var"], lay["gamma"], lay["beta"], training=False, eps=T.BN_EPS)
        else:
            assert bias and torch.equal(folded[l][1], torch.ones_like(folded[l][1]))
        w, scale, shift = folded[l]
        got = F.conv2d(x, w, None, stride=stride, padding=k // 2) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name


def test_macs_per_frame():
    from instag_amd import teeth as T
    # by hand: the stem at stride 2 and conv_seg at stride 4 of a 64 x 64 frame
    stem = (27 * 32 + 288 * 32 + 288 * 64) * 32 * 32
    assert sum(cin * (cout or 8) * k * k * 1024 for n, _, _, cin, cout, k, _ in T.LAYERS[:3]) == stem
    assert T.macs_per_frame(64, 64) * 64 == T.macs_per_frame(512, 512)
    assert T.macs_per_frame(512, 512, classes=9) - T.macs_per_frame(512, 512) == 128 * 128 * 128
    assert 40e9 < T.macs_per_frame() < 60e9


def test_teeth_torch_on_the_cpu(g15_weights):
    from instag_amd import teeth as T
    frames = H.seeded_frames(2, 64, 64, seed=2)
    mask = T.teeth_torch(g15_weights, frames)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (2, 64, 64) and set(mask.unique().tolist()) <= {0, 1}
    seg = T.TeethSegmenter(g15_weights, "cpu")
    logits, labels = seg.logits(frames), seg.labels(frames)
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (2, 8, 16, 16)
    assert torch.equal(labels, T.labels_torch(logits, 64, 64)) and torch.equal(seg.mask(frames), mask)
    assert torch.equal(mask, (labels == 7).to(torch.uint8)) and 0 < int(mask.sum()) < mask.numel() // 2
    # a frame's mask does not depend on its neighbours in the batch
    assert torch.equal(T.teeth_torch(g15_weights, frames[1:]), mask[1:])


def test_size_errors(g15_weights):
    from instag_amd import teeth as T
    seg = T.TeethSegmenter(g15_weights, "cpu")
    for shape in ((1, 64, 80, 3), (1, 32, 64, 3), (1, 96, 100, 3)):
        with pytest.raises(ValueError, match="multiples of 32"):
            seg.mask(torch.zeros(shape, dtype=torch.uint8))
        with pytest.raises(ValueError, match="multiples of 32"):
            T.teeth_torch(g15_weights, torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        seg.mask(torch.zeros(1, 64, 64, 3))
    with pytest.raises(ValueError, match="max_batch"):
        T.TeethSegmenter(g15_weights, "cpu", max_batch=0)


def test_teeth_identity_on_the_cpu(tmp_path, g15_weights):
    from PIL import Image
    from instag_amd import teeth as T
    os.makedirs(tmp_path / "ori_imgs")
    ids = (1, 2, 10)
    frames = H.seeded_frames(3, 64, 96, seed=5).numpy()
    for j, i in enumerate(ids):
        Image.fromarray(frames[j], "RGB").save(tmp_path / "ori_imgs" / f"{i}.jpg", quality=95)
    got = T.teeth_identity(str(tmp_path), g15_weights, device="cpu", batch=2)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 64, 96) and got.device.type == "cpu"
    assert sorted(os.listdir(tmp_path / "teeth_mask")) == ["1.npy", "10.npy", "2.npy"]
    decoded = np.stack([np.array(Image.open(tmp_path / "ori_imgs" / f"{i}.jpg").convert("RGB")) for i in ids])
    assert torch.equal(got, T.teeth_torch(g15_weights, torch.from_numpy(decoded)))       # numeric order: 1, 2, 10
    assert not torch.equal(got[1], got[2]) and int(got.sum()) > 0
    for j, i in enumerate(ids):
        arr = np.load(tmp_path / "teeth_mask" / f"{i}.npy")
        assert arr.dtype == np.bool_ and arr.shape == (64, 96)
        assert np.array_equal((arr != 0).astype(np.uint8), got[j].numpy())                 # as dataset.decode_images reads it
    # write=False leaves the directory alone
    os.remove(tmp_path / "teeth_mask" / "2.npy")
    again = T.teeth_identity(str(tmp_path), g15_weights, device="cpu", write=False)
    assert torch.equal(again, got) and not os.path.exists(tmp_path / "teeth_mask" / "2.npy")


def test_library_exports_the_entry_points_and_checks_arguments():
    from instag_amd import _lib
    lib = _lib.lib()
    for n in ("instag_teeth_workspace_bytes", "instag_teeth_forward", "instag_teeth_labels"):
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n)
    assert ctypes.sizeof(_lib.TeethWeights) == 3 * 71 * ctypes.sizeof(ctypes.c_void_p)       # struct instag_teeth_weights
    per_frame = lib.instag_teeth_workspace_bytes(1, 512, 512)
    assert 16 * 2 ** 20 * 6 <= per_frame <= 128 * 2 ** 20                # six stride-4 maps of 256 channels, and change
    assert lib.instag_teeth_workspace_bytes(3, 512, 512) == 3 * per_frame
    for bad in ((1, 64, 80), (1, 32, 64), (0, 64, 64), (1, 64, 8192)):
        assert lib.instag_teeth_workspace_bytes(*bad) == 0
        assert b"multiples of 32" in lib.instag_last_error()
    one = ctypes.c_void_p(256)
    s = _lib.TeethWeights()
    for l in range(71):
        s.w[l] = s.scale[l] = s.shift[l] = 256
    fwd = lambda *a: lib.instag_teeth_forward(*a)
    ok = (ctypes.byref(s), one, 1, 64, 64, 8, one, one, one, one, 1 << 30, None)

    def with_(**kw):
        names = ("w", "frames", "B", "H", "W", "C", "logits4", "labels", "mask", "workspace", "bytes", "stream")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    assert fwd(*with_(frames=None)) == 1 and b"NULL" in lib.instag_last_error()
    assert fwd(*with_(logits4=None, labels=None, mask=None)) == 1 and b"no output" in lib.instag_last_error()
    assert fwd(*with_(W=80)) == 1 and b"multiples of 32" in lib.instag_last_error()
    assert fwd(*with_(C=7)) == 1 and b"C in [8, 32]" in lib.instag_last_error()
    assert fwd(*with_(C=33)) == 1
    assert fwd(*with_(bytes=1024)) == 3 and b"workspace" in lib.instag_last_error()          # INSTAG_E_SPACE
    s.shift[70] = None
    assert fwd(*ok) == 1 and b"layer 70" in lib.instag_last_error()
    assert lib.instag_teeth_labels(None, 1, 64, 64, 8, one, one, None) == 1
    assert lib.instag_teeth_labels(one, 1, 64, 64, 8, None, None, None) == 1
    assert lib.instag_teeth_labels(one, 1, 64, 66, 8, one, None, None) == 1 and b"multiples of 4" in lib.instag_last_error()
    assert lib.instag_teeth_labels(one, 1, 64, 64, 7, one, None, None) == 1 and b"C in [8, 32]" in lib.instag_last_error()
