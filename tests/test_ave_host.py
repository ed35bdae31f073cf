"""CPU: the 'ave' audio extractor (AudioNet_ave, scene/motion_net.py:132-149) through the host-side layers: module
mirror against golden G8, checkpoints, the C ABI's four new symbols, the operator's stock-architecture check."""
import json
import os

import numpy as np
import pytest
import torch

from tests import ave_helpers as H

TAGS = [n[0] for n in H.NETWORKS]


@pytest.fixture(scope="module")
def g8(golden_dir):
    return np.load(f"{golden_dir}/g8_ave_nets.npz")


def _net(tag):
    from oracle.grid_torch import GridEncoder
    net, salt = H.build_network(tag, encoder_cls=GridEncoder)
    return H.load_closed_form(net, salt)


@pytest.mark.parametrize("tag", TAGS)
def test_ave_networks_construct_with_reference_layout(g8, tag):
    """The four networks build with audio_extractor='ave' and their state_dicts have the reference's names and shapes."""
    from instag_amd.motion_net import AudioNet_ave, audio_in_dim
    from oracle.grid_torch import GridEncoder
    net, _ = H.build_network(tag, encoder_cls=GridEncoder)
    assert isinstance(net.audio_net, AudioNet_ave) and audio_in_dim("ave") == 32
    layout = json.loads(bytes(g8["layout"]).decode())[tag]
    ours = sorted((k, list(v.shape)) for k, v in net.state_dict().items())
    assert ours == [(k, s) for k, s in layout]
    assert [k for k, _ in ours if k.startswith("audio_net.")] == [
        f"audio_net.encoder_fc1.{i}.{p}" for i in (0, 2, 4) for p in ("bias", "weight")]


@pytest.mark.parametrize("tag", TAGS)
def test_ave_mirror_matches_reference(g8, tag):
    """fp32 CPU forward and autograd of the mirror modules == the reference's fp64 results on the closed-form weights
    (the tolerance of the G5 / G7 comparisons in test_oracle_golden.py)."""
    net = _net(tag)
    a = torch.from_numpy(g8["a"].astype(np.float32))
    assert tuple(a.shape) == (8, 1, 512)
    enc_a = net.encode_audio(a)
    ref = torch.from_numpy(g8[f"{tag}.enc_a"])
    assert enc_a.shape == ref.shape and enc_a.dtype == torch.float32
    assert float((enc_a.detach().double() - ref).abs().max()) <= 1e-6 + 1e-5 * float(ref.abs().max())
    assert float(g8[f"{tag}.softmax"].max()) < 0.9               # the fixture's attention is not saturated
    (enc_a * H.enc_weights(net.audio_dim).float()).sum().backward()
    params = dict(net.named_parameters())
    for k in H.GRAD_KEYS:
        gref = torch.from_numpy(g8[f"{tag}.grad.{k}"])
        got = params[k].grad
        assert got.shape == gref.shape
        assert float((got.double() - gref).abs().max()) <= 1e-6 + 1e-5 * float(gref.abs().max()), (tag, k)


def test_ave_checkpoints_round_trip(tmp_path):
    """A reference-format checkpoint tuple with 'ave' audio tensors loads through load_pretrained_motion, and
    save_checkpoints writes the same tensors back; GaussianModel.capture / restore carry an 'ave' PMF."""
    from instag_amd.gaussian_model import GaussianModel
    from instag_amd.motion_net import MotionNetwork, PersonalizedMotionNetwork
    from instag_amd.pretrain import PretrainFaceTrainer, load_pretrained_motion
    args = H.ave_args("face")
    src = H.load_closed_form(MotionNetwork(args=args), 5)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    assert tuple(sd["audio_net.encoder_fc1.0.weight"].shape) == (256, 512)
    path = os.path.join(str(tmp_path), "chkpnt_face_latest.pth")
    torch.save((sd, {"state": {}, "param_groups": []}, 123), path)              # (motion_params, optimizer, iteration)
    ids = []
    for k in range(2):
        g = GaussianModel(1, neural_motion_grid=H.load_closed_form(PersonalizedMotionNetwork(args=args), 6 + k))
        g.create_random(32, "cpu", seed=k)
        ids.append(g)
    umf = load_pretrained_motion(MotionNetwork(args=args), path)
    for k, v in umf.state_dict().items():
        assert torch.equal(v, sd[k]), k
    tr = PretrainFaceTrainer(ids, umf, torch.tensor([0.0, 1.0, 0.0]), names=["a", "b"])
    tr.iteration = 9
    root = os.path.join(str(tmp_path), "out")
    tr.save_checkpoints(root)
    back, osd, it = torch.load(os.path.join(root, "chkpnt_face_latest.pth"), weights_only=False)
    assert it == 9 and set(back) == set(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    cap, usd, _, uit = torch.load(os.path.join(root, "a", "chkpnt_face_latest.pth"), weights_only=False)
    assert uit == 9 and len(cap) == 15 and set(usd) == set(sd)
    pmf_sd = ids[0].neural_motion_grid.state_dict()
    assert set(cap[14]) == set(pmf_sd)
    fresh = GaussianModel(1, neural_motion_grid=PersonalizedMotionNetwork(args=args))
    fresh.restore(cap)
    for k, v in fresh.neural_motion_grid.state_dict().items():
        assert torch.equal(v, pmf_sd[k]), k
    # a deepspeech network refuses the 'ave' tensors instead of dropping them
    from types import SimpleNamespace
    with pytest.raises(RuntimeError, match="encoder_fc1.4"):
        MotionNetwork(args=SimpleNamespace(audio_extractor="deepspeech", type="face")).load_state_dict(sd)


def test_ave_share_audio_net_still_raises():
    from instag_amd.pretrain import PretrainFaceTrainer
    with pytest.raises(NotImplementedError, match="share_audio_net"):
        PretrainFaceTrainer([], None, None, share_audio_net=True)


def test_ave_cabi_symbols():
    import ctypes
    from instag_amd import _lib
    lib = _lib.lib()
    for name in ("instag_frame_code_ave_saved_floats", "instag_frame_code_ave_forward",
                 "instag_frame_code_ave_backward_workspace_bytes", "instag_frame_code_ave_backward"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    assert lib.instag_abi_version() == 10
    # saved block: z1 [8][256], z2 [8][128], f2 [8][32], the attention stage's 8 * 32 + 280 floats
    assert lib.instag_frame_code_ave_saved_floats(32) == 8 * 256 + 8 * 128 + 8 * 32 + 8 * 32 + 280
    assert lib.instag_frame_code_ave_saved_floats(0) == -1
    assert lib.instag_frame_code_ave_saved_floats(4096) == -1           # the attention stage would not fit the LDS
    assert lib.instag_frame_code_ave_backward_workspace_bytes(32) == 0
    # argument errors are reported before any device work
    one = ctypes.c_void_p(16)
    params = (ctypes.c_void_p * 20)()
    assert lib.instag_frame_code_ave_forward(None, None, params, one, None, one, 32, None, None) != 0
    assert b"NULL tensor" in lib.instag_last_error()
    assert lib.instag_frame_code_ave_forward(one, None, params, one, None, one, 32, None, None) != 0
    assert b"NULL parameter" in lib.instag_last_error()
    assert lib.instag_frame_code_ave_backward(one, None, params, one, one, None, params, 4096, None, 0, None) != 0
    assert b"do not fit" in lib.instag_last_error()


def test_ave_supported_rejects_a_non_stock_head():
    """The HIP operator takes the stock AudioNet_ave only; anything else is answered by the torch modules."""
    from instag_amd import audio as A
    from instag_amd.motion_net import MotionNetwork, MouthMotionNetwork
    umf = MotionNetwork(args=H.ave_args("face"))
    params = A._module_params_ave(umf)
    assert len(params) == A.NPARAM_AVE == 20 and all(p is not None for p in params)
    assert params[0] is umf.audio_net.encoder_fc1[0].weight and params[5] is umf.audio_net.encoder_fc1[4].bias
    assert params[6] is umf.audio_att_net.attentionConvNet[0].weight and params[19] is umf.exp_encode_net.net[1].weight
    mouth = MouthMotionNetwork(args=H.ave_args("mouth"))
    assert A._module_params_ave(mouth)[18:] == [None, None]
    a = torch.randn(8, 1, 512)
    mouth.audio_net.encoder_fc1[2] = torch.nn.Linear(256, 128, bias=False)
    assert A._module_params_ave(mouth) is None and not A.supported(mouth, a, None)
    assert tuple(mouth.encode_audio(a).shape) == (1, 32)                 # the torch path still answers
    umf.audio_net.encoder_fc1[1] = torch.nn.LeakyReLU(0.2)
    assert A._module_params_ave(umf) is None
    # the deepspeech head is not taken for an 'ave' one
    from types import SimpleNamespace
    ds = MotionNetwork(args=SimpleNamespace(audio_extractor="deepspeech", type="face"))
    assert not A._is_ave(ds) and len(A._module_params(ds)) == 26
