"""CPU tests of instag_amd/ave_encoder.py: the torch statement against golden G9, the BatchNorm fold, the window
arithmetic, the feature array and the per-frame window, the state-dict forms, the mel front end against an independent
fp64 restatement, and the C symbols."""
import json
import math
import struct
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ave_encoder_helpers as H


@pytest.fixture(scope="module")
def g9(golden_dir):
    return np.load(f"{golden_dir}/g9_ave_encoder.npz")


@pytest.fixture(scope="module")
def weights():
    return H.weights()


def test_torch_statement_matches_g9(g9, weights):
    """audio_encoder_torch in fp64 on G9's mel == the reference module's recorded outputs (1e-9 of the scale), with the
    recorded liveness and state-dict layout."""
    from instag_amd import ave_encoder as A
    mel = torch.from_numpy(g9["mel"].astype(np.float32))
    assert tuple(mel.shape) == (H.G9_T, 80) and torch.equal(mel, H.seeded_mel(H.G9_T))
    starts = A.window_starts(H.G9_T)
    assert starts.dtype == torch.int32 and starts.tolist() == g9["starts"].tolist()
    windows = A.cut_windows(mel, starts)
    assert torch.equal(windows, H.reference_windows(mel))
    taps = []
    out = A.audio_encoder_torch(weights, windows.double(), taps)
    want = torch.from_numpy(g9["out"])
    scale = float(want.abs().max())
    err = float((out - want).abs().max())
    print(f"g9: err {err:.3e} scale {scale:.3e}")
    assert out.dtype == torch.float64 and tuple(out.shape) == (9, 512)
    assert err <= 1e-9 * scale
    assert np.allclose(H.liveness(taps), g9["positive"], atol=1e-12)
    assert all(0.25 <= p <= 0.75 for p in g9["positive"])
    layout = json.loads(bytes(g9["layout"]).decode())
    assert layout == sorted([k, list(v.shape)] for k, v in weights.state_dict().items())
    assert A.MACS_PER_WINDOW == sum(int(np.prod(t.shape[1:])) * ci * k * k
                                    for t, (ci, _, k, _, _, _) in zip(taps, A.LAYERS))


def test_folded_form_equals_unfolded(weights):
    """relu(scale * conv_nobias(x) + shift [+ x]) with the fp64 fold == the unfolded statement."""
    from instag_amd import ave_encoder as A
    x = A.cut_windows(H.seeded_mel(19, seed=1)).double()
    want = A.audio_encoder_torch(weights, x)
    for (w, scale, shift), (_, _, _, stride, pad, residual) in zip(weights.folded(torch.float64), A.LAYERS):
        y = F.conv2d(x, w, None, stride=stride, padding=pad) * scale[None, :, None, None] + shift[None, :, None, None]
        x = F.relu(y + x if residual else y)
    got = x.squeeze(2).squeeze(2)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert all(s.dtype == torch.float32 for _, s, _ in weights.folded(torch.float32))


def test_window_starts():
    from instag_amd import ave_encoder as A
    for T in (16, 17, 19, 40, 96, 100, 832):
        assert A.window_starts(T).tolist() == H.reference_starts(T), T
    assert A.window_starts(16).tolist() == [0, 0]
    with pytest.raises(ValueError):
        A.window_starts(15)


def _get_audio_features_mode2(features, index):
    """utils/audio_utils.py:38-73 restated."""
    left = index - 4
    right = index + 4
    pad_left = 0
    pad_right = 0
    if left < 0:
        pad_left = -left
        left = 0
    if right > features.shape[0]:
        pad_right = right - features.shape[0]
        right = features.shape[0]
    auds = features[left:right]
    if pad_left > 0:
        auds = torch.cat([torch.zeros_like(auds[:pad_left]), auds], dim=0)
    if pad_right > 0:
        auds = torch.cat([auds, torch.zeros_like(auds[:pad_right])], dim=0)
    return auds


def test_ave_features_and_frame_window(weights):
    from instag_amd import ave_encoder as A
    mel = H.seeded_mel(H.G9_T)
    feats = A.ave_features(mel, weights, "cpu")
    rows = A.audio_encoder_torch(weights, A.cut_windows(mel)).numpy()
    n = rows.shape[0]
    assert isinstance(feats, np.ndarray) and feats.dtype == np.float32 and feats.shape == (n + 4, 512, 1)
    assert np.array_equal(feats[2:-2, :, 0], rows)
    assert np.array_equal(feats[0], feats[2]) and np.array_equal(feats[1], feats[2])
    assert np.array_equal(feats[-1], feats[-3]) and np.array_equal(feats[-2], feats[-3])
    assert not np.array_equal(feats[2], feats[3])
    permuted = torch.from_numpy(feats).float().permute(0, 2, 1)
    for idx in (0, 3, n + 3):
        got = A.frame_window(feats, idx)
        assert tuple(got.shape) == (8, 1, 512) and got.dtype == torch.float32
        assert torch.equal(got, _get_audio_features_mode2(permuted, idx))
    assert float(A.frame_window(feats, 0)[:4].abs().max()) == 0 and float(A.frame_window(feats, n + 3)[-3:].abs().max()) == 0
    # the CPU operator is the torch statement
    enc = A.AudioEncoder(weights, "cpu")
    assert np.array_equal(enc.encode(mel).numpy(), rows)
    assert np.array_equal(enc.encode_windows(A.cut_windows(mel)).numpy(), rows)


def test_state_dict_forms(tmp_path, weights):
    from instag_amd.ave_encoder import AudioEncoderWeights
    sd = H.state_dict()
    assert len(sd) == 13 * 6 and "0.conv_block.0.weight" in sd and "12.conv_block.1.running_var" in sd
    prefixed = {f"audio_encoder.{k}": v for k, v in sd.items()}
    prefixed["audio_encoder.3.conv_block.1.num_batches_tracked"] = torch.tensor(7)
    for form in (sd, prefixed):
        w = AudioEncoderWeights.from_state_dict(form)
        for a, b in zip(w.layers, weights.layers):
            assert all(torch.equal(a[f], b[f]) for f in a)
    torch.save(sd, tmp_path / "enc.pth")
    w = AudioEncoderWeights.load(tmp_path / "enc.pth")
    assert torch.equal(w.layers[12]["var"], weights.layers[12]["var"])
    missing = dict(sd)
    del missing["6.conv_block.1.running_mean"]
    with pytest.raises(KeyError, match="layer 6"):
        AudioEncoderWeights.from_state_dict(missing)
    wrong = dict(sd)
    wrong["9.conv_block.0.weight"] = torch.zeros(256, 128, 3, 2)
    with pytest.raises(ValueError, match="layer 9"):
        AudioEncoderWeights.from_state_dict(wrong)
    lay = weights.to(dtype=torch.float64)
    assert lay[0]["gamma"].dtype == torch.float64
    for l in weights.layers:                       # the rule's BatchNorm statistics are not the identity
        assert 0.5 <= float(l["gamma"].min()) and float(l["gamma"].max()) <= 1.5
        assert 0.5 <= float(l["var"].min()) and float(l["var"].max()) <= 1.5
        assert float(l["mean"].abs().max()) > 0.1 and float(l["beta"].abs().max()) > 0.1


# ---- mel front end ---------------------------------------------------------------------------------------------------
def _slaney_hz_to_mel(f):
    return f / (200.0 / 3) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def _slaney_mel_to_hz(m):
    return m * (200.0 / 3) if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def _mel_basis_loop():
    """The 80-band Slaney basis band by band."""
    lo, hi = _slaney_hz_to_mel(55.0), _slaney_hz_to_mel(7600.0)
    pts = [_slaney_mel_to_hz(lo + (hi - lo) * i / 81.0) for i in range(82)]
    basis = np.zeros((80, 401))
    for b in range(80):
        left, centre, right = pts[b], pts[b + 1], pts[b + 2]
        for j in range(401):
            f = 8000.0 * j / 400.0
            if left < f <= centre:
                basis[b, j] = (f - left) / (centre - left)
            elif centre < f < right:
                basis[b, j] = (right - f) / (right - centre)
        basis[b] *= 2.0 / (right - left)
    return basis


def _melspectrogram_restated(x, pad_mode):
    x = np.asarray(x, dtype=np.float64)
    y = np.zeros_like(x)
    for t in range(len(x)):
        y[t] = x[t] - (0.97 * x[t - 1] if t > 0 else 0.0)
    if pad_mode == "constant":
        padded = np.concatenate([np.zeros(400), y, np.zeros(400)])
    else:
        padded = np.concatenate([y[1:401][::-1], y, y[-401:-1][::-1]])
    n = np.arange(800)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / 800.0)
    ang = 2.0 * np.pi * np.outer(np.arange(401), n) / 800.0
    cos_m, sin_m = np.cos(ang), np.sin(ang)
    frames = 1 + len(y) // 200
    mag = np.zeros((401, frames))
    for t in range(frames):
        seg = padded[200 * t:200 * t + 800] * hann
        mag[:, t] = np.sqrt((cos_m @ seg) ** 2 + (sin_m @ seg) ** 2)
    S = 20.0 * np.log10(np.maximum(1e-5, _mel_basis_loop() @ mag)) - 20.0
    return np.clip(8.0 * ((S + 100.0) / 100.0) - 4.0, -4.0, 4.0).T


def test_mel_basis_structure():
    from instag_amd.ave_encoder import mel_basis
    B = mel_basis()
    assert B.shape == (80, 401) and B.dtype == np.float64 and (B >= 0).all()
    freqs = np.linspace(0, 8000, 401)
    assert (B[:, freqs <= 55.0] == 0).all() and (B[:, freqs >= 7600.0] == 0).all()
    for row in B:                                  # a single triangle: rises to one peak, then falls, zero outside
        nz = np.nonzero(row)[0]
        assert len(nz) >= 1 and np.array_equal(nz, np.arange(nz[0], nz[-1] + 1))
        peak = int(row.argmax())
        assert (np.diff(row[nz[0]:peak + 1]) > 0).all() and (np.diff(row[peak:nz[-1] + 1]) < 0).all()
    assert np.abs(B - _mel_basis_loop()).max() <= 1e-12


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_melspectrogram_matches_restatement(pad_mode):
    """melspectrogram == the direct-DFT restatement within 1e-4 on the [-4, 4] scale; both clip ends occur."""
    from instag_amd.ave_encoder import melspectrogram
    rng = np.random.RandomState(5)
    t = np.arange(1400) / 16000.0
    chirp = 8.0 * np.sin(2 * np.pi * (150.0 * t + 0.5 * 40000.0 * t * t)) + 0.05 * rng.randn(1400)
    x = np.concatenate([chirp, np.zeros(600)])     # 2,000 samples: 11 frames, the last ones silent
    want = _melspectrogram_restated(x, pad_mode)
    got = melspectrogram(torch.from_numpy(x), pad_mode=pad_mode)
    assert tuple(got.shape) == (11, 80) and got.dtype == torch.float32
    err = float(np.abs(got.double().numpy() - want).max())
    print(f"mel {pad_mode}: err {err:.3e}")
    assert want.min() == -4.0 and want.max() == 4.0 and float((np.abs(want) < 4.0).mean()) > 0.5
    assert err <= 1e-4
    assert torch.equal(melspectrogram(torch.from_numpy(x).float(), pad_mode=pad_mode),
                       melspectrogram(x.astype(np.float32), pad_mode=pad_mode))
    with pytest.raises(ValueError):
        melspectrogram(torch.from_numpy(x), pad_mode="edge")


def test_load_wav16k(tmp_path):
    from instag_amd.ave_encoder import load_wav16k

    def write(path, rate, channels, samples):
        with wave.open(str(path), "wb") as f:
            f.setnchannels(channels)
            f.setsampwidth(2)
            f.setframerate(rate)
            f.writeframes(struct.pack(f"<{len(samples)}h", *samples))

    write(tmp_path / "a.wav", 16000, 2, [0, 16384, -32768, 0, 32767, 32767])
    got = load_wav16k(tmp_path / "a.wav")
    assert got.dtype == torch.float32 and torch.equal(got, torch.tensor([0.25, -0.5, 32767 / 32768.0]))
    write(tmp_path / "b.wav", 22050, 1, [0, 1])
    with pytest.raises(ValueError, match="22050"):
        load_wav16k(tmp_path / "b.wav")


def test_c_symbols_resolve():
    from instag_amd import _lib
    lib = _lib.lib()
    for name in ("instag_ave_encoder_max_batch", "instag_ave_encoder_workspace_bytes", "instag_ave_encoder_forward"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
    assert lib.instag_abi_version() == _lib.ABI_VERSION == 10
    B = lib.instag_ave_encoder_max_batch()
    assert B >= 128
    assert lib.instag_ave_encoder_workspace_bytes(B) >= 2 * B * 32 * 80 * 16 * 4
    assert lib.instag_ave_encoder_workspace_bytes(0) == 0 and lib.instag_ave_encoder_workspace_bytes(B + 1) == 0
    assert b"batch" in lib.instag_last_error()
    assert lib.instag_ave_encoder_forward(None, None, 16, None, 1, None, None, 0, None) != 0
    assert b"NULL" in lib.instag_last_error()
