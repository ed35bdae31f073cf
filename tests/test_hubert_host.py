"""CPU tests of instag_amd/hubert.py: the torch statement against golden G17, the utterance's normalisation, the clip
rule against a slow restatement, the features end to end, the loader and its errors, the
third header of the C ABI, the conditions the GPU tests put on their inputs, and the [N,1024,2] table on a 'hubert'
network."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from instag_amd import hubert as HU
from instag_amd import wav2vec as W
from tests import hubert_helpers as H


@pytest.fixture(scope="module")
def g17(golden_dir):
    return np.load(f"{golden_dir}/g17_hubert.npz")


def test_statement_matches_g17(g17):
    w = H.weights("S", int(g17["weights_seed"]))
    want = torch.from_numpy(g17["last_hidden_state"])
    got = HU.hubert_torch(w, torch.from_numpy(g17["input_values"]))
    assert got.dtype == torch.float64 and tuple(got.shape) == (1, 18, 128) == tuple(want.shape)
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())
    taps = []
    assert torch.equal(HU.hubert_torch(w, torch.from_numpy(g17["input_values"]), taps), got)
    assert taps[-1][0] == "hidden" and taps[-1][1] is not None and taps[0][0] == "conv0"


def test_normalise_utterance_matches_g17(g17):
    audio = torch.from_numpy(g17["audio"].astype(np.float32))[0]
    want = torch.from_numpy(g17["input_values"])[0]
    got = HU.normalise_utterance(audio)
    assert got.dtype == torch.float32 and tuple(got.shape) == (6130,)
    assert torch.equal(got, want.float())                           # fp64 inside, one rounding to fp32
    assert float((got.double() - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max())
    assert torch.equal(HU.normalise_utterance(audio.double().numpy()), got)
    with pytest.raises(ValueError):
        HU.normalise_utterance(audio[None])


CLIP_CASES = [(L, 1000) for L in (400, 719, 720, 319999, 320000, 320079, 320080, 320399, 320400, 640079, 960000)] + \
             [(L, 20) for L in (6400, 6479, 6480, 6799, 6800, 13000)]


@pytest.mark.parametrize("L,clip_rows", CLIP_CASES)
def test_clip_plan_matches_the_reference_loop(L, clip_rows):
    values = torch.arange(1, L + 1, dtype=torch.float64)
    plan, expected = HU.clip_plan(L, clip_rows)
    slow, slow_expected = H.slow_clips(values, clip_rows)
    assert expected == slow_expected == (L - 80) // 320
    assert len(plan) == len(slow)
    for (start, length), (clip, rows) in zip(plan, slow):
        assert torch.equal(values[start:start + length], clip), (L, start, length)
        assert W.frames_of(length) == rows and length >= 400
    assert sum(rows for _, rows in slow) == expected                # the reference's pad / truncate branch is never taken


def test_clip_plan_known_answers_and_errors():
    assert HU.clip_plan(960000) == ([(0, 320080), (320000, 320080), (640000, 320000)], 2999)
    assert [W.frames_of(n) for _, n in HU.clip_plan(960000)[0]] == [1000, 1000, 999]
    assert HU.clip_plan(320399) == ([(0, 320080)], 1000) and HU.clip_plan(320400) == ([(0, 320080), (320000, 400)], 1001)
    assert HU.clip_plan(320079) == ([(0, 320079)], 999)
    assert HU.CLIP_SAMPLES == 320080
    with pytest.raises(ValueError):
        HU.clip_plan(399)
    with pytest.raises(ValueError):
        HU.clip_plan(6400, clip_rows=1)
    for L in range(400, 20 * 320 * 3, 53):                          # the assertion inside holds on a sweep
        HU.clip_plan(L, 20)


@pytest.mark.parametrize("L,rows", [(13000, 40), (13330, 41)])
def test_hubert_features_cpu_end_to_end(L, rows):
    w = H.weights("S")
    wav = H.seeded_audio(1, L, seed=7)[0]
    feats = HU.hubert_features(wav, w, "cpu", clip_rows=20)
    values = HU.normalise_utterance(wav)
    clips, expected = H.slow_clips(values, 20)
    assert expected == rows
    out = torch.cat([HU.hubert_torch(w, c[None])[0] for c, _ in clips], dim=0)
    assert out.shape[0] == expected
    if out.shape[0] % 2 == 1:
        out = out[:-1]                                              # make_even_first_dim
    want = out.reshape(-1, 2, 128).numpy()
    assert feats.dtype == np.float32 and feats.shape == (rows // 2, 2, 128) == want.shape
    # The two full clips went through the statement as one batch, here one by one: the same fp32 arithmetic in another
    # blocking, so not the same bits (5.8e-7 and 5.2e-7 of the largest entry here).  Each is an fp32 statement of
    # config S, which sits at 3.6e-7 .. 8.3e-7 of the fp64 result on the cases of this suite (e32): two of them are
    # within 2 x 8.3e-7 of each other, rounded up to 2e-6.  One by one, below, the features are exact.
    assert float(np.abs(feats - want).max()) <= 2e-6 * float(np.abs(want).max())
    one_by_one = lambda wts, v: torch.cat([HU.hubert_torch(wts, r[None]) for r in v])      # noqa: E731
    assert np.array_equal(HU.hubert_features(wav, w, "cpu", encoder=one_by_one, clip_rows=20), want)
    assert np.array_equal(HU.hubert_features(wav, w, "cpu", encoder=HU.hubert_torch, clip_rows=20), feats)
    with pytest.raises(ValueError):
        HU.hubert_features(wav[:399], w, "cpu")


def test_loader_takes_both_prefixes_and_spellings(tmp_path):
    w = H.weights("O")
    assert "lm_head.weight" not in w.tensors and set(w.state_dict()) == {
        k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1")
        for k in w.tensors}
    for prefix, spelling in (("hubert.", "parametrizations"), ("", "weight_g")):
        sd = w.state_dict(prefix=prefix, weight_norm=spelling)
        assert all(k.startswith(prefix) for k in sd)
        sd["lm_head.weight"], sd["lm_head.bias"] = torch.zeros(32, 192), torch.zeros(32)
        sd[prefix + "masked_spec_embed"] = torch.zeros(192)
        sd[prefix + "encoder.unknown"] = torch.zeros(3)
        back = HU.HubertWeights.from_state_dict(sd, dict(H.O.hf(), vocab_size=32))
        assert back.tensors.keys() == w.tensors.keys() and back.dims.hidden == 192
        assert all(torch.equal(back.tensors[k], w.tensors[k]) and back.tensors[k].dtype == torch.float32 for k in w.tensors)
    torch.save(w.state_dict(prefix="hubert.", weight_norm="weight_g"), tmp_path / "pytorch_model.bin")
    config = {k: v for k, v in H.O.hf().items() if k != "vocab_size"}
    (tmp_path / "config.json").write_text(json.dumps(dict(config, architectures=["HubertForCTC"])))
    loaded = HU.HubertWeights.load(tmp_path)
    assert isinstance(loaded, HU.HubertWeights) and all(torch.equal(loaded.tensors[k], w.tensors[k]) for k in w.tensors)
    a, b, c = (HU.HubertWeights.random(H.S, s) for s in (5, 5, 6))
    assert all(torch.equal(a.tensors[k], b.tensors[k]) for k in a.tensors)
    assert not torch.equal(a.tensors["encoder.layer_norm.weight"], c.tensors["encoder.layer_norm.weight"])
    # vocab plays no part
    odd = W.Wav2Vec2Dims(**dict(H.S.__dict__, vocab=43))
    assert HU.HubertWeights.random(odd, 5).tensors.keys() == a.tensors.keys()
    with pytest.raises(ValueError, match="vocab"):
        W.Wav2Vec2Weights.random(odd, 5)
    # the common base: the shapes, the fold and the device layout are the wav2vec class's own functions
    assert HU.HubertWeights.pos_weight is W.Wav2Vec2Weights.pos_weight
    assert HU.HubertWeights.device_pack is W.Wav2Vec2Weights.device_pack


def test_loader_errors():
    w = H.weights("S")
    sd = w.state_dict()
    missing = {k: v for k, v in sd.items() if k != "encoder.layers.1.attention.k_proj.bias"}
    with pytest.raises(ValueError, match=r"encoder\.layers\.1\.attention\.k_proj\.bias"):
        HU.HubertWeights.from_state_dict(missing, H.S)
    bad = dict(sd)
    bad["feature_projection.projection.weight"] = torch.zeros(128, 60)
    with pytest.raises(ValueError, match=r"feature_projection\.projection\.weight.*\(128, 60\)"):
        HU.HubertWeights.from_state_dict(bad, H.S)
    for field, value in (("feat_proj_layer_norm", False), ("conv_pos_batch_norm", True), ("do_stable_layer_norm", False),
                         ("feat_extract_norm", "group")):
        with pytest.raises(ValueError, match=field):
            HU.HubertWeights.from_state_dict(sd, dict(H.S.hf(), **{field: value}))
    assert HU.HubertWeights.from_state_dict(sd, dict(H.S.hf(), feat_proj_layer_norm=True, conv_pos_batch_norm=False)).dims == H.S
    with pytest.raises(ValueError, match="heads"):
        HU.HubertWeights.random(W.Wav2Vec2Dims(**dict(H.S.__dict__, heads=4)))


def test_macs_without_the_head():
    d = W.Wav2Vec2Dims()
    assert W.macs(d, 22400) - W.macs(d, 22400, head=False) == 69 * d.hidden * d.vocab
    # per row of a long clip: every convolution's products at its rate per output row (strides 5,2,2,2,2,2,2 -> 64, 32,
    # 16, 8, 4, 2, 1 rows of layer l per row), the projection, the positional convolution, and per layer the four
    # hidden x hidden products, the two feed-forward products and the two attention products over T = 1000 keys
    conv = 64 * 512 * 10 + sum(r * 512 * 512 * k for r, k in zip((32, 16, 8, 4, 2, 1), (3, 3, 3, 3, 2, 2)))
    row = conv + 512 * 1024 + 1024 * 64 * 128 + 24 * (4 * 1024 * 1024 + 2 * 1024 * 4096 + 2 * 1000 * 1024)
    got = W.macs(d, 320080, head=False)
    assert abs(got - 1000 * row) <= 0.01 * 1000 * row, (got, 1000 * row)
    assert 2.04e9 < 2 * 1000 * 1000 * 1024 < 2.06e9                 # the attention's share of a layer, next to 12.6e9


def test_c_abi_of_the_third_header():
    """include/instag_hubert.h goes through the reader of instag_hip.h, told of the wav2vec header's struct; the library
    exports what it declares and refuses bad shapes before any device work (no GPU needed)."""
    from instag_amd import _cabi, _lib
    path = os.path.join(os.path.dirname(_cabi.HEADER), "instag_hubert.h")
    with pytest.raises(ValueError, match="instag_wav2vec_weights"):
        _cabi.read(path)                                            # the reader does not follow #include
    structs, protos, constants = _cabi.read(path, _lib._WAV2VEC_STRUCTS)
    assert structs == {} and constants == {"INSTAG_HUBERT_MAX_FRAMES": 1024} == _lib.HUBERT
    assert list(protos) == ["instag_hubert_workspace_bytes", "instag_hubert_taps_floats", "instag_hubert_forward",
                            "instag_hubert_attention"] == list(_lib._HUBERT_PROTOTYPES)
    weights_p = C.POINTER(_lib.Wav2vecWeights)
    assert protos["instag_hubert_workspace_bytes"] == (C.c_size_t, [weights_p, C.c_int32, C.c_int32])
    assert protos["instag_hubert_taps_floats"] == (C.c_size_t, [weights_p, C.c_int32, C.c_int32])
    assert protos["instag_hubert_forward"] == (C.c_int32, [weights_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                           C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p])
    assert protos["instag_hubert_attention"] == (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p])
    assert not set(protos) & set(_lib.EXPORTED_SYMBOLS)             # instag_hip.h's list is as it was
    with pytest.raises(ValueError, match="declared twice"):
        _cabi.parse("typedef struct instag_wav2vec_weights { int a; } instag_wav2vec_weights;", _lib._WAV2VEC_STRUCTS)
    L = _lib.lib()
    for name, (res, args) in protos.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args
    s = _lib.Wav2vecWeights()
    for field, value in H.S.__dict__.items():
        setattr(s, field, value)
    s.vocab = 0                                                     # plays no part
    assert L.instag_hubert_workspace_bytes(C.byref(s), 2, 320080) > 0
    assert L.instag_hubert_workspace_bytes(C.byref(s), 1, 400 + 320 * 1023) > 0
    for batch, n in ((1, 400 + 320 * 1024), (1, 399), (0, 320080)):
        assert L.instag_hubert_workspace_bytes(C.byref(s), batch, n) == 0
        assert b"INSTAG_HUBERT_MAX_FRAMES" in L.instag_last_error()
        assert L.instag_hubert_taps_floats(C.byref(s), batch, n) == 0
    rows = [4479, 2239, 1119, 559, 279, 139, 69]
    assert L.instag_hubert_taps_floats(C.byref(s), 2, 22400) == 2 * (sum(rows) * 64 + (2 + 2 * 2) * 69 * 128)
    s.heads = 3
    assert L.instag_hubert_workspace_bytes(C.byref(s), 1, 22400) == 0 and b"hidden / heads" in L.instag_last_error()
    s.heads = 2
    one = C.c_void_p(64)
    assert L.instag_hubert_forward(C.byref(s), None, 1, 22400, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
    assert b"NULL tensor" in L.instag_last_error()
    assert L.instag_hubert_forward(C.byref(s), one, 1, 400 + 320 * 1024, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
    assert b"INSTAG_HUBERT_MAX_FRAMES" in L.instag_last_error()
    assert L.instag_hubert_forward(C.byref(s), one, 1, 22400, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
    assert b"NULL weight in convolution 0" in L.instag_last_error()
    # everything set but the head: the weights pass, and the workspace (too short here) is looked at next
    for name, kind in s._fields_:
        if kind is C.c_void_p and name not in ("head_w", "head_b"):
            setattr(s, name, 64)
        elif kind is not C.c_int32 and kind is not C.c_void_p:
            setattr(s, name, kind(*([64] * len(kind()))))
    assert s.head_w is None and s.head_b is None and s.ln1_g[47] == 64
    assert L.instag_hubert_forward(C.byref(s), one, 1, 22400, one, one, 16, 0, None, None) == 3        # INSTAG_E_SPACE
    assert b"workspace smaller" in L.instag_last_error() and b"head" not in L.instag_last_error()
    assert L.instag_wav2vec_forward(C.byref(s), one, 1, 22400, one, one, 16, 0, None, None) == _lib.E_ARG     # vocab 0
    aligned = C.c_void_p(256)
    for frames, heads in ((0, 1), (1025, 1), (8, 0)):
        assert L.instag_hubert_attention(aligned, aligned, 1, frames, heads, None) == _lib.E_ARG
    assert b"hubert_attention" in L.instag_last_error()
    assert L.instag_hubert_attention(None, aligned, 1, 8, 1, None) == _lib.E_ARG


NETWORK_CASES = [("S", n) for n in (400, 719, 6130, 41200, 41520, 320000, 320080)] + [("O", n) for n in (400, 6130, 64400)]


@pytest.mark.parametrize("name,n", NETWORK_CASES)
def test_network_references_meet_the_input_conditions(name, n):
    """The conditions the GPU tests put on their inputs hold for the seeded weights and audio (fp64, CPU)."""
    c = H.case(name, n)
    assert c.T == (n - 400) // 320 + 1
    c.check_inputs()


def test_other_references_meet_the_input_conditions(g17):
    H.Case(H.weights("S", int(g17["weights_seed"])), torch.from_numpy(g17["input_values"]).float()).check_inputs()
    H.case("S", 64400, 3).check_inputs()
    for T, heads, B in H.ATTENTION_SHAPES:
        H.attention_case(T, heads, B).check_inputs()
    for T in (200, 1000):
        H.attention_case(T, 1, 1, crafted=True).check_inputs()
    for clip in H.features_wav()[1]:                                # the two clips of the features test
        clip.check_inputs()


def test_default_max_batch_at_the_real_size():
    """The workspace of a 320,080-sample clip at the real dimensions is about 240 MB, so four fit the 1 GiB limit; the
    entry only computes the size, so HubertEncoder's default needs neither weights nor a GPU."""
    from instag_amd import _lib
    s = _lib.Wav2vecWeights()
    for field, value in W.Wav2Vec2Dims().__dict__.items():
        setattr(s, field, value)
    one = _lib.lib().instag_hubert_workspace_bytes(C.byref(s), 1, HU.CLIP_SAMPLES)
    assert 230e6 < one < 250e6 and 4 * one <= W.WORKSPACE_LIMIT < 5 * one
    assert HU.default_max_batch(W.Wav2Vec2Dims()) == 4
    for field, value in H.S.__dict__.items():
        setattr(s, field, value)
    small = _lib.lib().instag_hubert_workspace_bytes(C.byref(s), 1, HU.CLIP_SAMPLES)
    assert HU.default_max_batch(H.S) * small <= W.WORKSPACE_LIMIT < (HU.default_max_batch(H.S) + 1) * small + 4096


class NoEncoder(torch.nn.Module):          # the tri-plane encoders play no part in the per-frame branch
    def __init__(self, **kw):
        super().__init__()
        self.output_dim = 12


def test_the_wide_table_drives_a_hubert_network():
    from instag_amd import audio as A
    from instag_amd import motion_net
    from instag_amd.dataset import POSTFIX, audio_table
    from instag_amd.frame_store import audio_window
    assert dict(motion_net._AUDIO_DIMS)["hubert"] == 1024 == W.Wav2Vec2Dims().hidden and POSTFIX["hubert"] == "_hu"
    feats = torch.randn(11, 2, 1024, generator=torch.Generator().manual_seed(2)).numpy()
    table = audio_table(None, "hubert", audio_features=feats)
    assert tuple(table.shape) == (11, 1024, 2) and torch.equal(table[3, :, 1], torch.from_numpy(feats[3, 1]))
    torch.manual_seed(3)
    net = motion_net.MotionNetwork(args=SimpleNamespace(audio_extractor="hubert", type="face"), encoder_cls=NoEncoder)
    e = torch.rand(6, generator=torch.Generator().manual_seed(4))
    for idx in (0, 5, 10):
        a = audio_window(table, idx)
        assert tuple(a.shape) == (8, 1024, 2)
        assert not A.supported(net, a, e)                           # the torch branch runs
        with torch.no_grad():
            enc = net.encode_frame(a, e)[0]
        assert bool(torch.isfinite(enc).all()) and float(enc.abs().max()) > 0
