"""GPU tests of the wav2vec 2.0 operator (csrc/wav2vec.hip) against golden G16 and the fp64 CPU statement: both small
configs at every run length that takes another path (one row, a row short of a tile, more than one tile of rows, the
longest run), every stage through the operator's debug taps, batch independence, tile independence and determinism bit
for bit, the frame bound, and the chain
wav -> features -> audio window -> frame codes of an 'esperanto' network.

Tolerance: e32 = max|fp32 torch statement on the CPU - fp64| / max|fp64| is measured on each test's own inputs and must
lie in (1e-8, 1e-4); the operator must be within 8 x e32 of the fp64 result (relative to its largest entry).  The
operator's arithmetic is fp32 like the statement's; the factor, the AudioEncoder's, covers the different K-summation
order: the GEMM adds every product of a row in one k-ordered chain, K up to 8192 in the positional convolution.  Every
test prints the operator's error beside e32 and the bar before it asserts.  Observed on an MI355X: e32 3.4e-7 .. 1.13e-6,
operator 6.9e-7 .. 1.72e-6, at most 2.6 x e32 (G16: e32 6.41e-7, operator 1.18e-6; config O at n = 22400: e32 1.13e-6,
operator 1.72e-6); stage by stage (configs S and O at n = 6130) the operator sits at 1.0 .. 2.3 x the stage's own e32,
conv0 5.1e-7 / 5.1e-7, positional 1.22e-6 / 7.8e-7, the last feed-forward 7.3e-7 / 6.2e-7 for S; the features of the
chain test differ from the torch chain's by about 5e-6 under a bound of 2.8e-5.

The attention condition (a row whose largest probability exceeds 2 / T) is checked where it can hold, T > 2: a softmax
row of one or two entries cannot exceed 2 / T >= 1."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import wav2vec_helpers as H

pytestmark = pytest.mark.gpu

FACTOR = 8.0
FWD_TOL = 2e-5                              # of test_ave_gpu.py: frame_codes against the fp64 modules


def _check(name, got, want, e32, scale):
    err = float((got.detach().double().cpu() - want).abs().max()) / scale
    print(f"{name}: operator {err:.3e} e32 {e32:.3e} bar {FACTOR * e32:.3e} scale {scale:.3e}")
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32
    assert err <= FACTOR * e32, (name, err, e32)


@pytest.fixture(scope="module")
def ops():
    """One operator per config, kept for the module."""
    from instag_amd.wav2vec import Wav2Vec2CTC
    return {name: Wav2Vec2CTC(H.weights(name), "cuda") for name in H.CONFIGS}


def test_logits_match_g16(golden_dir):
    from instag_amd.wav2vec import Wav2Vec2CTC
    g16 = np.load(f"{golden_dir}/g16_wav2vec.npz")
    w = H.weights("S", int(g16["weights_seed"]))
    audio = torch.from_numpy(g16["audio"].astype(np.float32))
    case = H.Case(w, audio)
    want = torch.from_numpy(g16["logits"])
    assert float((case.want - want).abs().max()) <= 1e-9 * float(want.abs().max())
    case.check_inputs()
    e32, scale = case.e32()
    got = Wav2Vec2CTC(w, "cuda").logits(audio.cuda())
    assert got.is_cuda and not got.requires_grad
    _check("g16", got, want, e32, scale)


@pytest.mark.parametrize("n", [400, 719, 3200, 6130, 22130, 22400])
@pytest.mark.parametrize("B", [1, 2])
def test_config_s_matches_fp64(ops, B, n):
    case = H.case("S", n)
    assert case.T == {400: 1, 719: 1, 3200: 9, 6130: 18, 22130: 68, 22400: 69}[n]
    case.check_inputs()
    e32, scale = case.e32(slice(0, B))
    got = ops["S"].logits(case.audio[:B].cuda())
    _check(f"S B={B} n={n}", got, case.want[:B], e32, scale)


@pytest.mark.parametrize("n", [400, 6130, 22400])
def test_config_o_matches_fp64(ops, n):
    case = H.case("O", n)
    case.check_inputs()
    e32, scale = case.e32()
    got = ops["O"].logits(case.audio.cuda())
    _check(f"O n={n}", got, case.want, e32, scale)


@pytest.mark.parametrize("name", ["S", "O"])
def test_every_stage_matches_fp64(ops, name):
    """The operator's debug taps against the statement's, stage by stage: each within 8 x that stage's own e32."""
    from instag_amd.wav2vec import wav2vec2_torch
    case = H.case(name, 6130)
    want = {k: v for k, v in case.taps if not k.endswith("attn_probs") and k != "logits"}
    taps32 = []
    wav2vec2_torch(case.w, case.audio.float(), taps32)
    got = []
    logits = ops[name].logits(case.audio.cuda(), taps=got)
    assert [k for k, _ in got] == list(want)
    assert torch.equal(logits, ops[name].logits(case.audio.cuda()))
    for (k, g), (_, s32) in zip(got, [kv for kv in taps32 if kv[0] in want]):
        scale = float(want[k].abs().max())
        e32 = float((s32.double() - want[k]).abs().max()) / scale
        assert 1e-8 < e32 < 1e-4, (k, e32)
        _check(f"{name} {k}", g, want[k], e32, scale)


def test_too_many_frames_is_an_argument_error(ops):
    from instag_amd import _lib
    bound = _lib.WAV2VEC["INSTAG_WAV2VEC_MAX_FRAMES"]
    n = 400 + 320 * bound                                   # bound + 1 frames
    with pytest.raises(ValueError, match="INSTAG_WAV2VEC_MAX_FRAMES"):
        ops["S"].logits(torch.zeros(1, n, device="cuda"))
    with pytest.raises(ValueError):
        ops["S"].logits(torch.zeros(1, 399, device="cuda"))
    w, L = ops["S"], _lib.lib()
    import ctypes as C
    one = torch.zeros(64, device="cuda")
    rc = L.instag_wav2vec_forward(C.byref(w._struct), _lib.ptr(one), 1, n, _lib.ptr(one), _lib.ptr(one), 4 * one.numel(), 0,
                                  None, _lib.current_stream())
    assert rc == _lib.E_ARG
    torch.cuda.synchronize()


def test_bits_do_not_depend_on_call_operator_batch_or_tile():
    """Two calls and a second operator give the same bits; segment b of a chunked call over max_batch + 1 segments
    (max_batch = 2) equals the single-segment call bit for bit; so does every GEMM tile."""
    from instag_amd.wav2vec import Wav2Vec2CTC
    case = H.case("S", 6130, 3)
    w, audio = case.w, case.audio.cuda()
    op = Wav2Vec2CTC(w, "cuda", max_batch=2)
    first = op.logits(audio).clone()
    assert torch.equal(first, op.logits(audio)) and float(first.abs().max()) > 0
    assert torch.equal(first, Wav2Vec2CTC(w, "cuda").logits(audio))
    for b in range(3):
        assert torch.equal(op.logits(audio[b:b + 1])[0], first[b]), b
    assert not torch.equal(first[0], first[2])
    for tile in (1, 2, 3):
        assert torch.equal(Wav2Vec2CTC(w, "cuda", tile=tile).logits(audio), first), tile
    e32, scale = case.e32()
    _check("chunked", first, case.want, e32, scale)


def test_a_smaller_call_keeps_the_workspace():
    """Three segments of 6130 samples in chunks of two (the chunk tail), then one of 400: the second call needs fewer
    bytes, so the workspace stays where it is; both results are a fresh operator's bit for bit."""
    from instag_amd.wav2vec import Wav2Vec2CTC
    w, big, small = H.weights("S"), H.seeded_audio(3, 6130, seed=6130).cuda(), H.seeded_audio(1, 400, seed=400).cuda()
    op = Wav2Vec2CTC(w, "cuda", max_batch=2)
    first = op.logits(big).clone()
    where, size = op._ws.data_ptr(), op._ws.numel()
    second = op.logits(small)
    assert op._ws.data_ptr() == where and op._ws.numel() == size
    assert tuple(first.shape) == (3, 18, 44) and tuple(second.shape) == (1, 1, 44) and float(second.abs().max()) > 0
    assert torch.equal(first, Wav2Vec2CTC(w, "cuda", max_batch=2).logits(big))
    assert torch.equal(second, Wav2Vec2CTC(w, "cuda", max_batch=2).logits(small))


class NoEncoder(torch.nn.Module):          # the tri-plane encoders play no part in the per-frame branch
    def __init__(self, **kw):
        super().__init__()
        self.output_dim = 12


def test_features_to_frame_codes():
    """esperanto_features -> audio table -> audio window -> frame_codes on an 'esperanto' network == the same chain with
    the torch statement (fp32, on the GPU) in place of the HIP operator.  Bound, as test_ave_encoder_gpu.py's: both are
    within 8 x e32 (the operator, tested above) and e32 (the statement) of the fp64 rows, so the windows differ by at
    most delta = 9 e32 scale per entry; enc_a moves by at most ||J||_inf delta to first order, J the Jacobian of enc_a
    in the window taken from the fp64 CPU modules (doubled for the softmax's curvature), plus frame_codes' own FWD_TOL
    for each of the two evaluations."""
    from instag_amd import audio as A
    from instag_amd.dataset import audio_table
    from instag_amd.frame_store import audio_window
    from instag_amd.motion_net import MotionNetwork
    from instag_amd.wav2vec import esperanto_features, segment_plan, wav2vec2_torch
    w = H.weights("S")
    wav = H.seeded_audio(1, 35000, seed=7)[0]
    # e32 and the scale over the runs of this wav
    e32, scale = 0.0, 0.0
    for s, z, n, _, _ in segment_plan(35000):
        seg = torch.cat([wav.new_zeros(z * 320), wav[s * 320: s * 320 + n - z * 320]])[None]
        e, sc = H.Case(w, seg).e32()
        e32, scale = max(e32, e), max(scale, sc)
    feats_h = esperanto_features(wav, w, "cuda")
    feats_t = esperanto_features(wav, w, "cuda", encoder=wav2vec2_torch)
    assert feats_h.shape == feats_t.shape == (55, 16, 44) and feats_h.dtype == np.float32
    delta = (FACTOR + 1.0) * e32 * scale
    diff = float(np.abs(feats_h - feats_t).max())
    print(f"features: diff {diff:.3e} bound {delta:.3e} (e32 {e32:.3e} scale {scale:.3e})")
    assert diff <= delta and float(np.abs(feats_t).max()) > 0
    torch.manual_seed(3)
    net64 = MotionNetwork(args=SimpleNamespace(audio_extractor="esperanto", type="face"), encoder_cls=NoEncoder).double()
    dev = MotionNetwork(args=SimpleNamespace(audio_extractor="esperanto", type="face"), encoder_cls=NoEncoder)
    dev.load_state_dict(net64.state_dict())
    dev = dev.float().cuda()
    e = torch.rand(6, generator=torch.Generator().manual_seed(4))
    table_h = audio_table(None, "esperanto", audio_features=feats_h)
    table_t = audio_table(None, "esperanto", audio_features=feats_t)
    assert tuple(table_h.shape) == (55, 44, 16)
    for idx in (0, 30):
        a_h, a_t = audio_window(table_h, idx), audio_window(table_t, idx)
        assert tuple(a_h.shape) == (8, 44, 16)
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
