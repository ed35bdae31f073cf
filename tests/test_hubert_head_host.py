"""CPU: the per-frame branch of a 'hubert' head (AudioNet at dim_in 1024 on windows [8, 1024, 2]) through the host-side
layers: module mirror against golden G18, the C ABI's three new symbols and their size query, the synthetic frame."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import hubert_head_helpers as H

TAGS = [n[0] for n in H.NETWORKS]
TOL = dict(rtol=1e-5, atol=1e-6)           # of the G5 / G7 / G8 comparisons


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(f"{golden_dir}/g18_hubert_head.npz")


def _net(tag):
    from oracle.grid_torch import GridEncoder
    net, salt = H.build_network(tag, encoder_cls=GridEncoder)
    return H.load_closed_form(net, salt)


@pytest.mark.parametrize("tag", TAGS)
def test_hubert_head_networks_construct_with_reference_layout(g18, tag):
    """The four networks build with audio_extractor='hubert'; their state_dicts have the reference's names and shapes,
    and the audio net is the stock AudioNet at 1024 -> 128 -> 128 -> 64 -> 64."""
    from instag_amd.motion_net import AudioNet, audio_in_dim
    from oracle.grid_torch import GridEncoder
    net, _ = H.build_network(tag, encoder_cls=GridEncoder)
    assert isinstance(net.audio_net, AudioNet) and audio_in_dim("hubert") == 1024 and net.audio_net.win_size == 16
    layout = json.loads(bytes(g18["layout"]).decode())[tag]
    ours = sorted((k, list(v.shape)) for k, v in net.state_dict().items())
    assert ours == [(k, s) for k, s in layout]
    shapes = dict((k, s) for k, s in ours)
    assert shapes["audio_net.encoder_conv.0.weight"] == [128, 1024, 3]
    assert [shapes[f"audio_net.encoder_conv.{i}.weight"][:2] for i in (2, 4, 6)] == [[128, 128], [64, 128], [64, 64]]
    assert sum(k in shapes for k in H.AUDIO_KEYS) == (26 if hasattr(net, "exp_encode_net") else 24)


@pytest.mark.parametrize("tag", TAGS)
def test_hubert_head_mirror_matches_reference(g18, tag):
    """fp32 CPU forward and autograd of the mirror modules == the reference's fp64 results on the closed-form
    weights."""
    net = _net(tag)
    a = torch.from_numpy(g18["a"].astype(np.float32))
    assert tuple(a.shape) == (8, 1024, 2)
    enc_a = net.encode_audio(a)
    ref = torch.from_numpy(g18[f"{tag}.enc_a"])
    assert enc_a.shape == ref.shape and enc_a.dtype == torch.float32
    assert float((enc_a.detach().double() - ref).abs().max()) <= TOL["atol"] + TOL["rtol"] * float(ref.abs().max())
    assert float(g18[f"{tag}.softmax"].max()) < 0.9               # the fixture's attention is not saturated
    (enc_a * H.enc_weights(net.audio_dim).float()).sum().backward()
    params = dict(net.named_parameters())
    for k in H.BIAS_KEYS + (H.CONV1_KEY,):
        gref = torch.from_numpy(g18[f"{tag}.grad.{k}"])
        got = params[k].grad[:gref.shape[0]]
        assert got.shape == gref.shape
        assert float((got.double() - gref).abs().max()) <= TOL["atol"] + TOL["rtol"] * float(gref.abs().max()), (tag, k)
    # the dead taps: torch's gradients are exactly zero
    gw = params[H.CONV1_KEY].grad
    assert int(torch.count_nonzero(gw[:, :, 0])) == 0 and int(torch.count_nonzero(gw[:, :, 1:])) > 0
    for i in (2, 4, 6):
        gw = params[f"audio_net.encoder_conv.{i}.weight"].grad
        assert int(torch.count_nonzero(gw[:, :, 0])) == 0 and int(torch.count_nonzero(gw[:, :, 2])) == 0


def test_hubert_head_convolutions_are_linear_layers():
    """encoder_conv.0 on a window of two samples == the flattened window against taps 1 and 2 (fp64)."""
    net = _net("umf").double()
    a = torch.randn(8, 1024, 2, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    conv = net.audio_net.encoder_conv[0]
    want = conv(a).squeeze(-1)
    got = a.reshape(8, 2048) @ conv.weight[:, :, 1:].reshape(128, 2048).t() + conv.bias
    assert float((want - got).abs().max()) <= 1e-12


def test_hubert_head_cabi_symbols():
    """The three symbols resolve, are declared in a header the reader derives prototypes from, answer the size query
    and refuse bad arguments before any device work."""
    from instag_amd import _cabi, _lib
    lib = _lib.lib()
    names = ["instag_frame_code_wide_saved_floats", "instag_frame_code_wide_forward", "instag_frame_code_wide_backward"]
    _, protos, constants = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_frame_code_wide.h"))
    assert list(protos) == names and constants == {}
    for name in names:
        fn = getattr(lib, name)
        assert fn.restype is protos[name][0] and list(fn.argtypes) == protos[name][1]
    assert protos[names[0]] == (ctypes.c_int64, [ctypes.c_int32] * 3)
    # the argument lists of the ave pair with (dim_in, mid, dim_aud) in dim_aud's place
    ave = _lib._PROTOTYPES
    for what in ("forward", "backward"):
        want = list(ave[f"instag_frame_code_ave_{what}"][1])
        i = want.index(ctypes.c_int32)
        assert protos[f"instag_frame_code_wide_{what}"][1] == want[:i] + [ctypes.c_int32] * 3 + want[i + 1:]
    # saved block: z1, z2 [8][128], z3, z4, f1 [8][64], f2 [8][32], the attention stage's 8 * 32 + 280 floats
    saved = lib.instag_frame_code_wide_saved_floats
    assert saved(1024, 128, 32) == 8 * (128 + 128 + 64 + 64 + 64 + 32) + 8 * 32 + 280
    for dims in ((1024, 128, 32), (256, 128, 32), (768, 128, 32), (512, 128, 64)):
        assert saved(*dims) > 0, dims
    for dims in ((1000, 128, 32), (1024, 32, 32), (1280, 128, 32), (0, 128, 32), (1024, 128, 0), (1024, 128, 4000),
                 (29, 32, 32)):
        assert saved(*dims) == -1, dims
    one = ctypes.c_void_p(16)
    params = (ctypes.c_void_p * 26)()
    assert lib.instag_frame_code_wide_forward(None, None, params, one, None, one, 1024, 128, 32, None, None) == _lib.E_ARG
    assert b"NULL tensor" in lib.instag_last_error()
    assert lib.instag_frame_code_wide_forward(one, None, params, one, None, one, 1024, 128, 32, None, None) == _lib.E_ARG
    assert b"NULL parameter" in lib.instag_last_error()
    assert lib.instag_frame_code_wide_forward(one, None, params, one, None, one, 1000, 128, 32, None, None) == _lib.E_ARG
    assert b"dim_in must be" in lib.instag_last_error()
    assert lib.instag_frame_code_wide_backward(one, None, params, one, one, None, params, 1024, 32, 32, None, 0,
                                               None) == _lib.E_ARG
    assert b"mid 128" in lib.instag_last_error()


def test_hubert_head_supported_answers_false_without_a_device_or_a_stock_head():
    """On the CPU the torch modules answer; a head that is not the stock AudioNet is not taken."""
    from instag_amd import audio as A
    from instag_amd.motion_net import MouthMotionNetwork
    mouth = MouthMotionNetwork(args=H.hubert_args("mouth"))
    a = torch.randn(8, 1024, 2)
    assert not A.supported(mouth, a, None)
    assert len(A._module_params(mouth)) == 26 and A._module_params(mouth)[24:] == [None, None]
    assert tuple(mouth.encode_audio(a).shape) == (1, mouth.audio_dim)
    mouth.audio_net.win_size = 8
    assert A._module_params(mouth) is None
    assert A._WIDE.name == "frame_code_wide" and not A._WIDE.workspace


def test_synthetic_frame_hubert_changes_only_the_audio_window():
    from instag_amd.scene_synth import synthetic_frame
    for kw in (dict(), dict(priors=True, background=True)):
        base = synthetic_frame(32, 3, **kw)
        hub = synthetic_frame(32, 3, audio_extractor="hubert", **kw)
        assert set(base) == set(hub)
        assert tuple(hub["auds"].shape) == (8, 1024, 2) and hub["auds"].dtype == torch.float32
        for k in base:
            if k != "auds":
                assert torch.equal(base[k], hub[k]), k
    assert torch.equal(hub["auds"], synthetic_frame(32, 3, audio_extractor="hubert")["auds"])
    assert not torch.equal(hub["auds"], synthetic_frame(32, 4, audio_extractor="hubert")["auds"])
    assert 0.9 < float(hub["auds"].std()) < 1.1
