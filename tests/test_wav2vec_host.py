"""CPU tests of instag_amd/wav2vec.py: the torch statement against golden G16 and (where it imports) ``transformers``,
the streaming rule against a slow restatement and known answers, the window layout, the loader and its errors."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from instag_amd import wav2vec as W
from tests import wav2vec_helpers as H

KNOWN = {0: (1, 0, 1), 1600: (1, 4, 3), 18880: (1, 58, 30), 19200: (2, 59, 30), 19520: (2, 60, 31), 34930: (3, 107, 54),
         35000: (3, 109, 55), 35200: (3, 109, 55), 960000: (60, 2999, 1500), 960007: (60, 2999, 1500)}


@pytest.fixture(scope="module")
def g16(golden_dir):
    return np.load(f"{golden_dir}/g16_wav2vec.npz")


def test_statement_matches_g16(g16):
    w = H.weights("S", int(g16["weights_seed"]))
    sd = w.state_dict()
    assert sorted(sd) == list(g16["names"])
    assert [",".join(str(s) for s in sd[k].shape) for k in sorted(sd)] == list(g16["shapes"])
    audio = torch.from_numpy(g16["audio"].astype(np.float64))
    want = torch.from_numpy(g16["logits"])
    got = W.wav2vec2_torch(w, audio)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, 69, 44)
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())
    e32 = float((W.wav2vec2_torch(w, audio.float()).double() - want).abs().max()) / float(want.abs().max())
    assert abs(e32 - float(g16["e32"])) <= 0.5 * float(g16["e32"])


@pytest.mark.parametrize("spelling", ["parametrizations", "weight_g"])
def test_statement_matches_transformers_config_o(spelling):
    """Config O on odd lengths against a freshly built module; the old weight-norm spelling goes through the loader."""
    try:
        from transformers import Wav2Vec2Config, Wav2Vec2FeatureExtractor, Wav2Vec2ForCTC
    except ImportError as e:
        pytest.skip(f"transformers does not import: {e}")
    w = H.weights("O")
    if spelling == "weight_g":
        old = w.state_dict(weight_norm="weight_g")
        assert "wav2vec2.encoder.pos_conv_embed.conv.weight_g" in old
        w = W.Wav2Vec2Weights.from_state_dict(old, H.O.hf())
    config = Wav2Vec2Config(**H.O.hf(), hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0,
                            feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
                            mask_feature_prob=0.0)
    model = Wav2Vec2ForCTC(config).double().eval()
    missing = model.load_state_dict({k: v.double() for k, v in w.state_dict().items()}, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("masked_spec_embed") for k in missing.missing_keys)
    for n in (719, 6131, 22131):
        audio = H.seeded_audio(2, n, seed=n).double()
        values = torch.from_numpy(np.stack(Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm([r.numpy() for r in audio], None)))
        with torch.no_grad():
            want = model(input_values=values).logits
        got = W.wav2vec2_torch(w, audio)
        assert tuple(got.shape) == (2, W.frames_of(n), 44) == tuple(want.shape)
        assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max()), n


def _segment(audio, run):
    s, z, n, _, _ = run
    return torch.cat([audio.new_zeros(z * 320), audio[s * 320: s * 320 + n - z * 320]])


def test_segment_plan_matches_the_slow_restatement():
    for n in range(0, 320 * 125, 37):
        audio = torch.arange(1, n + 1, dtype=torch.float64)
        plan, slow = W.segment_plan(n), H.slow_runs(audio)
        assert len(plan) == len(slow), n
        for run, (seg, left, right) in zip(plan, slow):
            assert run[2] == seg.numel() and (run[3], run[4]) == (left, right), (n, run)
            assert torch.equal(_segment(audio, run), seg), (n, run)
            assert run[2] <= W.RUN_SAMPLES and W.frames_of(run[2]) == (run[2] - 400) // 320 + 1 <= 69


@pytest.mark.parametrize("n", sorted(KNOWN))
def test_segment_plan_known_answers(n):
    plan = W.segment_plan(n)
    M = sum(right - left for *_, left, right in plan)
    assert (len(plan), M, M // 2 + 1) == KNOWN[n]
    if n == 34930:
        assert plan[1][2:] == (22130, 10, 59) and W.frames_of(22130) == 68
        assert plan[2][2:] == (6130, 10, 18)


@pytest.mark.parametrize("M", [0, 1, 4, 59, 109])
def test_unfold_rows_is_f_unfold(M):
    rows = torch.randn(M, 44, generator=torch.Generator().manual_seed(M))
    got = W.unfold_rows(rows)
    assert tuple(got.shape) == (M // 2 + 1, 16, 44)
    if M > 0:            # the reference: [M,44] -> [1,44,M,1] -> unfold (16,1), padding (8,0), stride (2,1) -> [n,16,44]
        u = F.unfold(rows.t()[None, :, :, None], kernel_size=(16, 1), padding=(8, 0), stride=(2, 1))
        want = u.reshape(44, 16, -1).permute(2, 1, 0)
        assert torch.equal(got, want)
    else:
        assert float(got.abs().max()) == 0.0


def test_loader_errors():
    w = H.weights("S")
    sd = w.state_dict()
    missing = {k: v for k, v in sd.items() if k != "wav2vec2.encoder.layers.1.attention.k_proj.bias"}
    with pytest.raises(ValueError, match=r"encoder\.layers\.1\.attention\.k_proj\.bias"):
        W.Wav2Vec2Weights.from_state_dict(missing, H.S)
    bad = dict(sd)
    bad["lm_head.weight"] = torch.zeros(40, 128)
    with pytest.raises(ValueError, match=r"lm_head\.weight.*\(40, 128\)"):
        W.Wav2Vec2Weights.from_state_dict(bad, H.S)
    for field, value in (("do_stable_layer_norm", False), ("feat_extract_norm", "group"), ("conv_bias", False),
                         ("hidden_act", "relu"), ("feat_extract_activation", "gelu_new"), ("conv_stride", [5, 2, 2, 2, 2, 2, 1])):
        with pytest.raises(ValueError, match=field):
            W.Wav2Vec2Weights.from_state_dict(sd, dict(H.S.hf(), **{field: value}))
    base = {k: v for k, v in H.S.hf().items() if k not in ("do_stable_layer_norm", "feat_extract_norm", "conv_bias")}
    with pytest.raises(ValueError, match="do_stable_layer_norm"):          # transformers' defaults are the base variant
        W.dims_of(base)
    for field, value in (("heads", 4), ("conv_dim", 72), ("intermediate", 250), ("pos_kernel", 127), ("pos_groups", 8),
                         ("layers", 0), ("vocab", 43)):
        with pytest.raises(ValueError, match=field):
            W.Wav2Vec2Weights.random(W.Wav2Vec2Dims(**dict(H.S.__dict__, **{field: value})))
    for dims in (H.S, H.O, W.Wav2Vec2Dims()):
        assert dims.check() is dims and W.dims_of(dims.hf()) == dims


def test_round_trip_and_ignored_keys(tmp_path):
    w = H.weights("O")
    for prefix, spelling in (("wav2vec2.", "parametrizations"), ("", "weight_g")):
        sd = w.state_dict(prefix=prefix, weight_norm=spelling)
        sd[prefix + "masked_spec_embed"] = torch.zeros(192)
        sd[prefix + "feature_extractor.conv_layers.0.layer_norm.num_batches_tracked"] = torch.tensor(3)
        back = W.Wav2Vec2Weights.from_state_dict(sd, H.O.hf())
        assert back.dims == H.O and back.tensors.keys() == w.tensors.keys()
        assert all(torch.equal(back.tensors[k], w.tensors[k]) and back.tensors[k].dtype == torch.float32 for k in w.tensors)
    torch.save(w.state_dict(weight_norm="weight_g"), tmp_path / "pytorch_model.bin")
    (tmp_path / "config.json").write_text(json.dumps(dict(H.O.hf(), architectures=["Wav2Vec2ForCTC"])))
    loaded = W.Wav2Vec2Weights.load(tmp_path)
    assert all(torch.equal(loaded.tensors[k], w.tensors[k]) for k in w.tensors)
    # the fold: w = g v / ||v|| over dims (0, 1) per tap, what torch's weight_norm(dim=2) computes
    v, g = w.tensors["encoder.pos_conv_embed.conv.weight_v"].double(), w.tensors["encoder.pos_conv_embed.conv.weight_g"].double()
    assert torch.allclose(w.pos_weight(), torch._weight_norm(v, g, 2), rtol=1e-14, atol=0)
    assert os.path.exists(tmp_path / "config.json")


def test_random_is_seeded_and_macs():
    a, b, c = W.Wav2Vec2Weights.random(H.S, 5), W.Wav2Vec2Weights.random(H.S, 5), W.Wav2Vec2Weights.random(H.S, 6)
    assert all(torch.equal(a.tensors[k], b.tensors[k]) for k in a.tensors)
    assert not torch.equal(a.tensors["lm_head.weight"], c.tensors["lm_head.weight"])
    assert 24.5e9 < W.macs(W.Wav2Vec2Dims()) < 26e9                        # about 25 GMAC per 1.4 s of audio
    assert sum(int(np.prod(s)) for s in W._shapes(W.Wav2Vec2Dims()).values()) // 10 ** 6 == 315


def test_c_abi_of_the_second_header():
    """include/instag_wav2vec.h goes through the reader of instag_hip.h; the library exports what it declares and refuses
    bad shapes before any device work (no GPU needed)."""
    import ctypes as C
    from instag_amd import _cabi, _lib
    structs, protos, constants = _cabi.read(os.path.join(os.path.dirname(_cabi.HEADER), "instag_wav2vec.h"))
    assert list(structs) == ["instag_wav2vec_weights"] and _lib.Wav2vecWeights._fields_ == structs["instag_wav2vec_weights"]._fields_
    assert C.sizeof(_lib.Wav2vecWeights) == 8 * 4 + (4 * 7 + 10 + 12 * 48) * 8
    assert _lib.Wav2vecWeights.conv_w.offset == 32 and _lib.Wav2vecWeights.ln1_g.offset == 32 + 38 * 8
    assert list(protos) == ["instag_wav2vec_workspace_bytes", "instag_wav2vec_taps_floats", "instag_wav2vec_forward"]
    assert len(protos["instag_wav2vec_forward"][1]) == 10
    assert constants["INSTAG_WAV2VEC_MAX_LAYERS"] == 48 == _lib.Wav2vecWeights.ln1_g.size // 8
    L = _lib.lib()
    s = _lib.Wav2vecWeights()
    for field, value in H.S.__dict__.items():
        setattr(s, field, value)
    assert L.instag_wav2vec_workspace_bytes(C.byref(s), 2, 22400) > 0
    bound = constants["INSTAG_WAV2VEC_MAX_FRAMES"]
    assert L.instag_wav2vec_workspace_bytes(C.byref(s), 1, 400 + 320 * (bound - 1)) > 0
    for batch, n in ((1, 399), (0, 22400), (1, 400 + 320 * bound)):
        assert L.instag_wav2vec_workspace_bytes(C.byref(s), batch, n) == 0
        assert b"INSTAG_WAV2VEC_MAX_FRAMES" in L.instag_last_error()
    s.heads = 3
    assert L.instag_wav2vec_workspace_bytes(C.byref(s), 1, 22400) == 0 and b"hidden / heads" in L.instag_last_error()
    assert L.instag_wav2vec_taps_floats(C.byref(s), 1, 22400) == 0
    one = C.c_void_p(64)
    assert L.instag_wav2vec_forward(C.byref(s), one, 1, 22400, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
    s.heads = 2
    # the seven convolution blocks, then projection, positional and two per layer
    rows = [4479, 2239, 1119, 559, 279, 139, 69]
    assert L.instag_wav2vec_taps_floats(C.byref(s), 2, 22400) == 2 * (sum(rows) * 64 + (2 + 2 * 2) * 69 * 128)
    assert L.instag_wav2vec_forward(C.byref(s), None, 1, 22400, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
    assert b"NULL tensor" in L.instag_last_error()
    assert L.instag_wav2vec_forward(C.byref(s), one, 1, 22400, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
    assert b"NULL weight in convolution 0" in L.instag_last_error()


def test_reference_meets_the_input_conditions():
    """The conditions the GPU tests put on their inputs hold for the seeded weights and audio (fp64, CPU)."""
    for name, n in (("S", 22400), ("S", 3200), ("O", 6130)):
        H.case(name, n).check_inputs()


def test_esperanto_features_cpu_end_to_end():
    w = H.weights("S")
    wav = H.seeded_audio(1, 35000, seed=7)[0]
    feats = W.esperanto_features(wav, w, "cpu")
    assert feats.dtype == np.float32 and feats.shape == (55, 16, 44)
    rows = []
    for seg, left, right in H.slow_runs(wav):
        rows.append(W.wav2vec2_torch(w, seg[None])[0, left:right])
    rows = torch.cat(rows)
    assert rows.shape[0] == 109
    want = W.unfold_rows(rows).numpy()
    # the full runs went through the statement as one batch, here one by one: the same arithmetic in another blocking
    assert float(np.abs(feats - want).max()) <= 1e-5 * float(np.abs(want).max())
    assert np.array_equal(feats[0, :8], np.zeros((8, 44), np.float32)) and float(np.abs(feats[0, 8]).max()) > 0
    assert np.array_equal(W.esperanto_features(wav, w, "cpu", encoder=W.wav2vec2_torch), feats)
    assert W.esperanto_features(torch.zeros(0), w, "cpu").shape == (1, 16, 44)
