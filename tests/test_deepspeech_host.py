"""CPU tests of instag_amd/deepspeech.py: the MFCC front end piece by piece (DCT against scipy, the filterbank's
triangles, the frame, step, row and window counts, the eps rule), the input rows, the interpolation and the two
windowing loops against a literal transcription, the recurrence against ``torch.nn.LSTM`` with the weights remapped,
the clip, the reader of frozen graphs on synthetic files, the .npz route, the features end to end on a CPU device and
the fourth header of the C ABI.  Nothing here is compared with a TensorFlow run: neither TensorFlow nor the frozen graph
was at hand."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from instag_amd import deepspeech as D
from tests import deepspeech_helpers as H

LENGTHS = (399, 400, 401, 560, 561, 16000, 16001, 47999)


def seeded_wav(L, seed=11):
    g = np.random.default_rng(seed + L)
    t = np.arange(L) / 16000.0
    return (3000 * np.sin(2 * np.pi * 220 * t) + 1500 * np.sin(2 * np.pi * 1310 * t + 1) + g.normal(0, 200, L)).astype(np.int16)


def test_dct_matches_scipy():
    import scipy.fftpack
    x = np.random.default_rng(1).normal(size=(7, 26))
    want = scipy.fftpack.dct(x, type=2, axis=1, norm="ortho")
    assert np.abs(x @ D.dct_matrix(26) - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(D.dct_matrix(26).T @ D.dct_matrix(26) - np.eye(26)).max() <= 1e-13          # orthonormal


def test_filterbank_is_26_triangles():
    fb, b = D.filterbank(), D.mel_bins()
    assert fb.shape == (26, 257) and b.shape == (28,) and b[0] == 0 and b[-1] == 256 and np.all(np.diff(b) >= 0)
    assert np.all(np.diff(b)[5:] > 0)                                # (bins may coincide only at the low end)
    for j in range(26):
        lo, peak, hi = int(b[j]), int(b[j + 1]), int(b[j + 2])
        assert np.all(fb[j, :lo] == 0) and np.all(fb[j, hi:] == 0) and np.all(fb[j] >= 0) and np.all(fb[j] <= 1)
        if lo < peak < hi:
            assert fb[j, peak] == 1.0 and fb[j, lo] == 0.0
            assert np.all(np.diff(fb[j, lo:peak + 1]) > 0) and np.all(np.diff(fb[j, peak:hi]) < 0)
            assert np.allclose(np.diff(fb[j, lo:peak + 1]), 1.0 / (peak - lo), rtol=0, atol=1e-15)
        elif peak < hi:                                              # bin[j] == bin[j+1]: only the falling side
            assert fb[j, peak] == 1.0
    assert sum(1 for j in range(26) if int(b[j]) < int(b[j + 1]) < int(b[j + 2])) >= 24


@pytest.mark.parametrize("L", LENGTHS)
def test_counts_follow_the_formulas(L):
    F = 1 if L <= 400 else 1 + math.ceil((L - 400) / 160)
    S = math.ceil(F / 2)
    N = int(round(L / 16000 * 50))
    W = max(0, math.ceil((N - 1) / 2))
    wav = seeded_wav(L)
    assert (D.n_frames(L), D.n_steps(L), D.n_rows(L), D.n_windows(L)) == (F, S, N, W)
    m = D.mfcc_features(wav)
    assert m.shape == (F, 26) and m.dtype == np.float64 and np.isfinite(m).all()
    x = D.input_vectors(wav)
    assert x.shape == (S, 494) and x.dtype == np.float32
    rows = D.interpolate(np.random.default_rng(L).normal(size=(S, 29)), L)
    assert rows.shape == (N, 29) and rows.dtype == np.float64
    assert D.windows(rows).shape == (W, 16, 29)


def test_mfcc_pieces():
    """Coefficient 0 is the log of the frame's energy; the others follow from the filterbank, the DCT and the lifter,
    recomputed here frame by frame."""
    import scipy.fftpack
    wav = seeded_wav(1234)
    m = D.mfcc_features(wav)
    s = wav.astype(np.float64)
    s = np.concatenate([s[:1], s[1:] - 0.97 * s[:-1]])
    s = np.concatenate([s, np.zeros((m.shape[0] - 1) * 160 + 400 - len(s))])
    for f in (0, 3, m.shape[0] - 1):
        power = np.abs(np.fft.rfft(s[160 * f:160 * f + 400], 512)) ** 2 / 512
        assert m[f, 0] == pytest.approx(np.log(power.sum()), rel=1e-12)
        cep = scipy.fftpack.dct(np.log(D.filterbank() @ power), type=2, norm="ortho") * (1 + 11 * np.sin(np.pi * np.arange(26) / 22))
        assert np.abs(m[f, 1:] - cep[1:]).max() <= 1e-10 * np.abs(cep).max()


def test_all_zero_signal_is_finite():
    m = D.mfcc_features(np.zeros(1000, dtype=np.int16))
    assert m.shape == (5, 26) and np.isfinite(m).all()
    assert np.all(m[:, 0] == np.log(np.finfo(np.float64).eps))       # the eps rule, on the energy and on the filters
    with pytest.raises(ValueError):
        D.mfcc_features(np.zeros((2, 100), dtype=np.int16))


def test_input_vectors_are_the_context_windows():
    wav = seeded_wav(5000)
    m = D.mfcc_features(wav)
    x = D.input_vectors(wav).astype(np.float64)
    S = x.shape[0]
    raw = np.zeros((S, 19, 26))
    for t in range(S):
        for c in range(19):
            r = 2 * (t + c - 9)
            if 0 <= t + c - 9 < S:
                raw[t, c] = m[r]
    mean, std = raw.mean(), math.sqrt(((raw - raw.mean()) ** 2).mean())
    want = ((raw - mean) / std).reshape(S, 494)
    assert np.abs(x - want).max() <= 2.0 ** -23 * np.abs(want).max()
    assert np.abs(x[0, :26] - (0 - mean) / std).max() <= 1e-6                 # out of range: the normalised zero
    assert abs(x.mean()) <= 1e-6 and abs(x.std() - 1) <= 1e-6


def test_interpolate_and_windows():
    logits = np.random.default_rng(3).normal(size=(3, 29))
    rows = D.interpolate(logits, 1600)                                # N = 5 > S = 3
    assert rows.shape == (5, 29)
    assert np.array_equal(rows[:3], logits) and np.array_equal(rows[3], logits[2]) and np.array_equal(rows[4], logits[2])
    assert np.array_equal(D.interpolate(logits, 640), logits[:2])    # N < S
    for N in (0, 1, 2, 3, 16, 17, 50):
        ramp = (np.arange(N * 29, dtype=np.float64) + 1).reshape(N, 29)
        want = H.reference_windows(ramp)
        got = D.windows(ramp)
        assert got.shape == (max(0, math.ceil((N - 1) / 2)), 16, 29)
        if want.size:
            assert np.array_equal(got, want)
        else:
            assert got.shape[0] == 0
    got = D.windows((np.arange(50 * 29, dtype=np.float64) + 1).reshape(50, 29))
    assert np.all(got[:, :, 0] != 50 * 29 - 28)                       # the last row is what the first loop drops


@pytest.mark.parametrize("S", [1, 2, 5])
def test_recurrence_matches_torch_lstm(S):
    w = H.weights("T")
    d = w.dims
    h3 = torch.randn(S, d.hidden, generator=torch.Generator().manual_seed(S), dtype=torch.float64)
    xp = torch.stack([h3 @ wx + b for wx, _, b in w.lstm_kernels("cpu", torch.float64)], dim=1)
    got = D.lstm_torch(w, xp)
    with torch.no_grad():
        want = H.torch_lstm(w)(h3[:, None])[0][:, 0]
    assert tuple(got.shape) == (S, 2 * d.cell) == tuple(want.shape)
    assert float((got - want).abs().max()) <= 1e-14
    assert float(want.abs().max()) > 1e-3
    taps = []
    x = H.seeded_rows(S, d.n_in).double()
    out = D.deepspeech_torch(w, x, taps)
    assert [n for n, _ in taps] == ["h1", "h2", "h3", "lstm", "h5", "logits"] and tuple(out.shape) == (S, d.n_out)
    with torch.no_grad():
        assert float((dict(taps)["lstm"] - H.torch_lstm(w)(dict(taps)["h3"][:, None])[0][:, 0]).abs().max()) <= 1e-14
    assert float((H.torch_chain(w, "cpu", torch.float64)(x) - out).abs().max()) <= 1e-13


def test_clip_is_exercised():
    w = H.scaled(H.weights("T"), "h1", 60.0)
    taps = []
    D.deepspeech_torch(w, H.seeded_rows(5, 494).double(), taps)
    h1 = dict(taps)["h1"]
    assert float(h1.max()) == 20.0 and int((h1 == 20.0).sum()) >= 3 and float(h1.min()) == 0.0
    plain = []
    D.deepspeech_torch(H.weights("T"), H.seeded_rows(5, 494).double(), plain)
    assert float(dict(plain)["h1"].max()) < 20.0


@pytest.mark.parametrize("mode", ["content", "float_val", "unpacked"])
@pytest.mark.parametrize("scope", ["", "deepspeech/"])
def test_graph_reader_returns_the_arrays(tmp_path, mode, scope):
    w = H.weights("T")
    path = tmp_path / "graph.pb"
    H.write_graph(path, w, mode, scope)
    consts = D.read_graph_consts(path)
    assert len(consts) == 16 and scope + "unrelated/ones" in consts and consts[scope + "Reshape/shape"][1] is None
    assert "input_node" not in consts and "logits" not in consts
    got = D.DeepSpeechWeights.load(path, w.dims)
    assert set(got.arrays) == set(w.arrays)
    for name, a in w.arrays.items():
        assert got.arrays[name].dtype == np.float32 and np.array_equal(got.arrays[name], a), name


def test_graph_reader_takes_the_other_spellings(tmp_path):
    w = H.weights("T")
    names = {"fw_kernel": "rnn/fw/lstm_cell/weights", "fw_bias": "rnn/fw/lstm_cell/biases",
             "bw_kernel": "rnn/bw/lstm_cell/weights", "bw_bias": "rnn/bw/lstm_cell/biases"}
    H.write_graph(tmp_path / "g.pb", w, "content", names=names)
    got = D.DeepSpeechWeights.load(tmp_path / "g.pb", w.dims)
    assert all(np.array_equal(got.arrays[n], a) for n, a in w.arrays.items())


def test_graph_reader_lists_the_consts_when_it_fails(tmp_path):
    w = H.weights("T")
    H.write_graph(tmp_path / "missing.pb", w, "content", leave_out=("h5", "bw_bias"))
    with pytest.raises(ValueError) as e:
        D.DeepSpeechWeights.load(tmp_path / "missing.pb", w.dims)
    text = str(e.value)
    assert "h5" in text and "bw_bias" in text and "no Const node by that name" in text
    for listed in ("unrelated/ones [3, 2]", "bidirectional_rnn/fw/basic_lstm_cell/kernel [24, 32]", "h1 [494, 16]", "b6 [29]"):
        assert listed in text, listed
    H.write_graph(tmp_path / "shape.pb", w, "content", reshape={"h2": (8, 32)})
    with pytest.raises(ValueError, match=r"h2 \(16, 16\): not the shape of h2 \(8, 32\)") as e:
        D.DeepSpeechWeights.load(tmp_path / "shape.pb", w.dims)
    assert "h2 [8, 32]" in str(e.value)
    with pytest.raises(ValueError, match="not the shape of"):       # the real dims against the tiny file
        D.DeepSpeechWeights.load(tmp_path / "shape.pb")
    (tmp_path / "empty.pb").write_bytes(b"")
    with pytest.raises(ValueError):
        D.DeepSpeechWeights.load(tmp_path / "empty.pb")


def test_npz_round_trip(tmp_path):
    w = D.DeepSpeechWeights.random(D.DeepSpeechDims(n_in=20, hidden=16, cell=8, n_out=5, clip=6.0, forget_bias=0.5), 4)
    w.save_npz(tmp_path / "w.npz")
    got = D.DeepSpeechWeights.load(tmp_path / "w.npz")
    assert got.dims == w.dims
    assert all(np.array_equal(got.arrays[n], a) for n, a in w.arrays.items())
    plain = D.DeepSpeechWeights.from_arrays(w.arrays)
    assert plain.dims == D.DeepSpeechDims(n_in=20, hidden=16, cell=8, n_out=5)
    arrays = dict(w.arrays)
    del arrays["b3"]
    with pytest.raises(ValueError, match="b3"):
        D.DeepSpeechWeights.from_arrays(arrays)
    arrays["b3"] = np.zeros(17, dtype=np.float32)
    with pytest.raises(ValueError, match="b3"):
        D.DeepSpeechWeights.from_arrays(arrays)


def test_dims_check_names_the_field():
    D.DeepSpeechDims().check()
    for name in H.CONFIGS:
        H.CONFIGS[name].check()
    for field, value in (("cell", 8), ("cell", 384), ("cell", 8192), ("hidden", 48), ("hidden", 0), ("n_in", 0),
                         ("n_out", 0), ("n_out", 2000), ("clip", 0.0)):
        with pytest.raises(ValueError, match=field):
            D.DeepSpeechDims(**{field: value}).check()
    with pytest.raises(ValueError, match="hidden = 16 is not supported"):
        D.DeepSpeechWeights.random(H.TINY, 1).device_pack("cpu")


def test_features_on_a_cpu_device():
    from instag_amd.dataset import audio_table
    w = H.weights("T")
    L = 8000
    wav = torch.from_numpy(seeded_wav(L).astype(np.float32) / 32768.0)
    assert np.array_equal(D.to_int16(wav), seeded_wav(L))
    assert np.array_equal(D.to_int16(torch.tensor([1.0, -1.0, 0.99999, -0.00001])), np.array([32767, -32768, 32767, 0]))
    feats = D.deepspeech_features(wav, w, "cpu")
    W = D.n_windows(L)
    assert feats.shape == (W, 16, 29) == (12, 16, 29) and feats.dtype == np.float64 and np.isfinite(feats).all()
    rows = D.input_vectors(seeded_wav(L))
    logits = D.deepspeech_torch(w, torch.from_numpy(rows)).double().numpy()
    assert np.array_equal(feats, H.reference_windows(D.interpolate(logits, L)))
    seen = []
    again = D.deepspeech_features(wav, w, "cpu", encoder=lambda ww, x: seen.append(tuple(x.shape)) or D.deepspeech_torch(ww, x))
    assert seen == [(25, 494)] and np.array_equal(again, feats)
    table = audio_table(None, "deepspeech", audio_features=feats)
    assert tuple(table.shape) == (W, 29, 16) and table.dtype == torch.float32
    assert torch.equal(table[3, :, 9], torch.from_numpy(feats[3, 9]).float())
    with pytest.raises(ValueError, match="sample rate"):
        D.deepspeech_features(wav, w, "cpu", sample_rate=44100)
    with pytest.raises(ValueError):
        D.deepspeech_features(wav[None], w, "cpu")


def test_default_max_rows_keeps_the_workspace_within_the_limit():
    from instag_amd import _lib
    s = _lib.DeepspeechWeights()
    for field, value in D.DeepSpeechDims().__dict__.items():
        setattr(s, field, value)
    L = _lib.lib()
    assert D.default_max_rows(D.DeepSpeechDims(), 3000) == 3000       # a minute of audio is one block, under 300 MB
    assert L.instag_deepspeech_workspace_bytes(C.byref(s), 3000, 3000) < 300 << 20
    for S in (30000, 60000):
        R = D.default_max_rows(D.DeepSpeechDims(), S)
        assert 1 <= R < S
        assert L.instag_deepspeech_workspace_bytes(C.byref(s), S, R) <= D.WORKSPACE_LIMIT
        assert L.instag_deepspeech_workspace_bytes(C.byref(s), S, R + 64) > D.WORKSPACE_LIMIT - (8 << 20)


def test_c_abi_of_the_deepspeech_header():
    """include/instag_deepspeech.h goes through the reader of instag_hip.h; the library exports what it declares and
    refuses bad shapes before any device work (no GPU needed)."""
    from instag_amd import _cabi, _lib
    path = os.path.join(os.path.dirname(_cabi.HEADER), "instag_deepspeech.h")
    structs, protos, constants = _cabi.read(path)
    assert list(structs) == ["instag_deepspeech_weights"] and _lib.DeepspeechWeights.__name__ == "DeepspeechWeights"
    assert constants == {"INSTAG_DEEPSPEECH_MAX_CELL": 4096, "INSTAG_DEEPSPEECH_MAX_STEPS": 1 << 20} == _lib.DEEPSPEECH
    assert list(protos) == ["instag_deepspeech_workspace_bytes", "instag_deepspeech_taps_floats", "instag_deepspeech_forward",
                            "instag_deepspeech_lstm"] == list(_lib._DEEPSPEECH_PROTOTYPES)
    fields = [n for n, _ in _lib.DeepspeechWeights._fields_]
    assert fields[:6] == ["n_in", "hidden", "cell", "n_out", "clip", "forget_bias"] and len(fields) == 19
    assert dict(_lib.DeepspeechWeights._fields_)["clip"] is C.c_float and dict(_lib.DeepspeechWeights._fields_)["wh"] is C.c_void_p
    weights_p = C.POINTER(_lib.DeepspeechWeights)
    assert _lib._DEEPSPEECH_PROTOTYPES["instag_deepspeech_workspace_bytes"] == (C.c_size_t, [weights_p, C.c_int32, C.c_int32])
    assert _lib._DEEPSPEECH_PROTOTYPES["instag_deepspeech_lstm"] == (
        C.c_int32, [weights_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])
    assert not set(protos) & set(_lib.EXPORTED_SYMBOLS)             # instag_hip.h's list is as it was
    L = _lib.lib()
    for name, (res, args) in _lib._DEEPSPEECH_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype == res and list(fn.argtypes) == args

    def struct_of(**kw):
        s = _lib.DeepspeechWeights()
        for field, value in {**H.CONFIGS["A"].__dict__, **kw}.items():
            setattr(s, field, value)
        return s

    s = struct_of()
    # the pieces: cell states, [S, 2 cell], S rows of 512 + 64 + 64 and of 8 cell, every piece rounded up to 64 floats
    assert L.instag_deepspeech_workspace_bytes(C.byref(s), 5, 5) == 4 * (512 + 2560 + 2560 + 320 + 320 + 10240)
    assert L.instag_deepspeech_workspace_bytes(C.byref(s), 5, 9) == L.instag_deepspeech_workspace_bytes(C.byref(s), 5, 5)
    assert L.instag_deepspeech_workspace_bytes(C.byref(s), 5, 2) == 4 * (512 + 2560 + 4 * 512 + 256 + 256 + 2 * 2048)
    assert L.instag_deepspeech_taps_floats(C.byref(s), 5) == 5 * (4 * 64 + 512)
    for steps, rows in ((0, 1), (5, 0), ((1 << 20) + 1, 1)):
        assert L.instag_deepspeech_workspace_bytes(C.byref(s), steps, rows) == 0
        assert b"INSTAG_DEEPSPEECH_MAX_STEPS" in L.instag_last_error()
    one = C.c_void_p(256)
    for kw, word in ((dict(cell=8), b"cell"), (dict(cell=384), b"cell"), (dict(cell=8192), b"cell"), (dict(hidden=48), b"hidden"),
                     (dict(n_in=0), b"n_in"), (dict(n_out=0), b"n_out"), (dict(clip=0.0), b"clip")):
        bad = struct_of(**kw)
        assert L.instag_deepspeech_workspace_bytes(C.byref(bad), 5, 5) == 0 and word in L.instag_last_error()
        assert L.instag_deepspeech_taps_floats(C.byref(bad), 5) == 0
        assert L.instag_deepspeech_forward(C.byref(bad), one, 5, 5, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
        assert word in L.instag_last_error()
    assert L.instag_deepspeech_lstm(C.byref(struct_of(cell=8)), one, one, one, 5, None) == _lib.E_ARG
    assert L.instag_deepspeech_forward(C.byref(s), None, 5, 5, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
    assert b"NULL tensor" in L.instag_last_error()
    assert L.instag_deepspeech_forward(C.byref(s), one, 5, 5, one, one, 1 << 30, 4, None, None) == _lib.E_ARG
    assert L.instag_deepspeech_forward(C.byref(s), one, 5, 5, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
    assert b"NULL weight" in L.instag_last_error()
    for name, kind in s._fields_:
        if kind is C.c_void_p:
            setattr(s, name, 256)
    assert L.instag_deepspeech_forward(C.byref(s), one, 5, 5, one, one, 16, 0, None, None) == 3        # INSTAG_E_SPACE
    assert b"workspace smaller" in L.instag_last_error()
    s.wh = 260
    assert L.instag_deepspeech_forward(C.byref(s), one, 5, 5, one, one, 1 << 30, 0, None, None) == _lib.E_ARG
    assert b"16-byte" in L.instag_last_error()
    assert L.instag_deepspeech_lstm(C.byref(s), one, one, one, 5, None) == _lib.E_ARG and b"16-byte" in L.instag_last_error()
    s.wh = 256
    assert L.instag_deepspeech_lstm(C.byref(s), one, one, one, 0, None) == _lib.E_ARG
    assert L.instag_deepspeech_lstm(C.byref(s), None, one, one, 5, None) == _lib.E_ARG
