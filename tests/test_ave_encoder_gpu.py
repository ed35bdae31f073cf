"""GPU tests of the AudioEncoder operator (csrc/ave_encoder.hip) against golden G9 and the fp64 CPU statement: batch
sizes and edge tiles, the window gather, batch independence and determinism bit for bit, and the chain
wav features -> frame window -> frame codes of an 'ave' network.

Tolerance: e32 = max|fp32 torch statement on the CPU - fp64| / max|fp64| is measured on each test's own inputs, and the
operator must be within 8 x e32 of the fp64 result (relative to its largest entry).  The operator's arithmetic is fp32
like the statement's; the factor covers the different K-summation order of the MFMA tiles over K <= 2304 and the fold
of BatchNorm into one fp32 scale and shift per channel.  Every test prints the operator's error beside e32 and the bar
before it asserts.  Observed on an MI355X: e32 4.2e-7 .. 6.2e-7, operator 2.7e-7 .. 3.9e-7 (G9: e32 4.87e-7, operator
3.42e-7)."""
import numpy as np
import pytest
import torch

from tests import ave_encoder_helpers as H
from tests import ave_helpers

pytestmark = pytest.mark.gpu

FACTOR = 8.0
FWD_TOL = 2e-5                              # of test_ave_gpu.py: frame_codes against the fp64 modules


def _reference(weights, windows):
    """fp64 statement on the CPU, and e32 of the fp32 statement on the same inputs."""
    from instag_amd.ave_encoder import audio_encoder_torch
    taps = []
    want = audio_encoder_torch(weights, windows.double(), taps)
    scale = float(want.abs().max())
    e32 = float((audio_encoder_torch(weights, windows.float()).double() - want).abs().max()) / scale
    assert 1e-8 < e32 < 1e-5, e32
    return want, e32, scale, taps


def _check(name, got, want, e32, scale):
    err = float((got.detach().double().cpu() - want).abs().max()) / scale
    print(f"{name}: operator {err:.3e} e32 {e32:.3e} bar {FACTOR * e32:.3e} scale {scale:.3e}")
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32
    assert err <= FACTOR * e32, (name, err, e32)


@pytest.fixture(scope="module")
def g9(golden_dir):
    return np.load(f"{golden_dir}/g9_ave_encoder.npz")


@pytest.fixture(scope="module")
def g9_weights():
    return H.weights()


@pytest.fixture(scope="module")
def random_case():
    """Other weights than G9's and seven windows, with their fp64 reference (computed once)."""
    from instag_amd.ave_encoder import cut_windows
    w = H.weights(seed=3)
    windows = cut_windows(H.seeded_mel(34, seed=2))
    assert windows.shape[0] == 7
    return (w, windows) + _reference(w, windows)


def test_encode_matches_g9(g9, g9_weights):
    from instag_amd.ave_encoder import AudioEncoder, cut_windows
    mel = torch.from_numpy(g9["mel"].astype(np.float32))
    want = torch.from_numpy(g9["out"])
    ref, e32, scale, _ = _reference(g9_weights, cut_windows(mel))
    assert float((ref - want).abs().max()) <= 1e-9 * scale
    got = AudioEncoder(g9_weights, "cuda").encode(mel.cuda())
    assert got.is_cuda and not got.requires_grad
    _check("g9", got, want, e32, scale)


@pytest.mark.parametrize("B", [1, 3, 7])
def test_encode_windows_matches_fp64(random_case, B):
    from instag_amd.ave_encoder import AudioEncoder
    w, windows, want, e32, scale, taps = random_case
    assert all(0.25 <= p <= 0.75 for p in H.liveness(taps)), H.liveness(taps)
    assert float((want == 0).double().mean()) > 0.05 and float((want > 0).double().mean()) > 0.05
    got = AudioEncoder(w, "cuda").encode_windows(windows[:B].cuda())
    _check(f"B={B}", got, want[:B], e32, scale)


@pytest.mark.parametrize("T", [16, 19])
def test_encode_short_mels(g9_weights, T):
    from instag_amd.ave_encoder import AudioEncoder, cut_windows
    mel = H.seeded_mel(T, seed=T)
    want, e32, scale, _ = _reference(g9_weights, cut_windows(mel))
    assert want.shape[0] == 2
    got = AudioEncoder(g9_weights, "cuda").encode(mel.cuda())
    _check(f"T={T}", got, want, e32, scale)
    if T == 16:
        assert torch.equal(got[0], got[1])                    # both windows are clamped to start 0


def test_batch_independence_bitwise(g9_weights):
    """One chunked call over max_batch + 1 windows: the rows of window 0, max_batch - 1 (the last of the first chunk)
    and max_batch (alone in the second chunk) equal single-window calls bit for bit, and meet the fp64 bar."""
    from instag_amd.ave_encoder import AudioEncoder, cut_windows, window_starts
    enc = AudioEncoder(g9_weights, "cuda")
    mb = enc.max_batch
    T = 16 + (mb - 1) * 80 // 25
    while window_starts(T).numel() < mb + 1:
        T += 1
    starts = window_starts(T)
    assert starts.numel() == mb + 1
    mel = H.seeded_mel(T, seed=11)
    rows = enc.encode(mel.cuda())
    assert tuple(rows.shape) == (mb + 1, 512)
    pick = [0, mb - 1, mb]
    windows = cut_windows(mel, starts[pick])
    for j, i in enumerate(pick):
        single = enc.encode_windows(windows[j:j + 1].cuda())
        assert torch.equal(single[0], rows[i]), i
    want, e32, scale, _ = _reference(g9_weights, windows)
    _check("chunked", rows[pick], want, e32, scale)
    assert not torch.equal(rows[0], rows[mb])


def test_a_smaller_call_keeps_the_workspace(g9_weights):
    """max_batch + 1 windows (the chunk tail), then one: the second call needs fewer bytes, so the workspace stays
    where it is; both results are a fresh operator's bit for bit."""
    from instag_amd.ave_encoder import AudioEncoder, cut_windows
    enc = AudioEncoder(g9_weights, "cuda")
    seven = cut_windows(H.seeded_mel(34, seed=2))
    big = seven[torch.arange(enc.max_batch + 1) % 7].contiguous().cuda()
    first = enc.encode_windows(big).clone()
    where, size = enc._ws.data_ptr(), enc._ws.numel()
    second = enc.encode_windows(big[:1])
    assert enc._ws.data_ptr() == where and enc._ws.numel() == size
    assert tuple(first.shape) == (enc.max_batch + 1, 512) and float(second.abs().max()) > 0
    assert torch.equal(first, AudioEncoder(g9_weights, "cuda").encode_windows(big))
    assert torch.equal(second, AudioEncoder(g9_weights, "cuda").encode_windows(big[:1]))
    assert torch.equal(second[0], first[0]) and torch.equal(first[enc.max_batch], first[enc.max_batch % 7])


def test_two_calls_same_bits(g9, g9_weights):
    from instag_amd.ave_encoder import AudioEncoder
    mel = torch.from_numpy(g9["mel"].astype(np.float32)).cuda()
    enc = AudioEncoder(g9_weights, "cuda")
    first = enc.encode(mel).clone()
    assert torch.equal(first, enc.encode(mel)) and float(first.abs().max()) > 0
    assert torch.equal(first, AudioEncoder(g9_weights, "cuda").encode(mel))


class NoEncoder(torch.nn.Module):          # the tri-plane encoders play no part in the per-frame branch
    def __init__(self, **kw):
        super().__init__()
        self.output_dim = 12


def test_features_to_frame_codes(g9, g9_weights):
    """ave_features -> frame_window -> frame_codes on an 'ave' network == the same chain with the torch statement in
    place of the HIP encoder.  Bound: both encoders are within 8 x e32 (the operator, tested above) and e32 (the
    statement) of the fp64 rows, so the windows differ by at most delta = 9 e32 scale per entry; enc_a moves by at
    most ||J||_inf delta to first order, J the Jacobian of enc_a in the window taken from the fp64 CPU modules
    (doubled for the softmax's curvature), plus frame_codes' own FWD_TOL for each of the two evaluations."""
    from instag_amd import audio as A
    from instag_amd.ave_encoder import audio_encoder_torch, ave_features, cut_windows, frame_window
    mel = torch.from_numpy(g9["mel"].astype(np.float32))
    _, e32, scale, _ = _reference(g9_weights, cut_windows(mel))
    feats_h = ave_features(mel, g9_weights, "cuda")
    feats_t = ave_features(mel, g9_weights, "cuda", encoder=audio_encoder_torch)
    assert feats_h.shape == feats_t.shape == (13, 512, 1) and feats_h.dtype == np.float32
    delta = (FACTOR + 1.0) * e32 * scale
    assert float(np.abs(feats_h - feats_t).max()) <= delta
    torch.manual_seed(3)
    net, _ = ave_helpers.build_network("umf", encoder_cls=NoEncoder)
    e = torch.rand(6, generator=torch.Generator().manual_seed(4))
    net64 = net.double()
    dev = ave_helpers.build_network("umf", encoder_cls=NoEncoder)[0]
    dev.load_state_dict(net64.state_dict())
    dev = dev.float().cuda()
    for idx in (0, 6):
        a_h, a_t = frame_window(feats_h, idx), frame_window(feats_t, idx)
        assert tuple(a_h.shape) == (8, 1, 512)
        J = torch.autograd.functional.jacobian(lambda a: net64.encode_frame(a, e.double())[0].reshape(-1), a_t.double())
        gain = float(J.reshape(J.shape[0], -1).abs().sum(1).max())
        assert A.supported(dev, a_h.cuda(), e.cuda())
        with torch.no_grad():
            enc_h = A.frame_codes(dev, a_h.cuda(), e.cuda())[0]
            enc_t = A.frame_codes(dev, a_t.cuda(), e.cuda())[0]
        size = max(1.0, float(enc_t.abs().max()))
        err = float((enc_h - enc_t).abs().max())
        bound = 2.0 * gain * delta + 2.0 * FWD_TOL * size
        print(f"frame {idx}: enc_a err {err:.3e} bound {bound:.3e} (gain {gain:.3e} delta {delta:.3e} size {size:.3e})")
        assert err <= bound
        assert float(enc_t.abs().max()) > 0
