"""device_op.DeviceOperator on the CPU: the chunk loop, the return-code checkers, the one workspace rule, the taps cut,
the CPU-path filter and the ``max_batch`` refusals of the operators built on it.  A stub stands in for a network: its
launch records what the loop hands it."""
import pytest
import torch

from instag_amd import _lib
from instag_amd.device_op import DeviceOperator


class Stub(DeviceOperator):
    def __init__(self, max_batch=2, check="check_arg", codes=()):
        super().__init__(None, "cpu")
        self.max_batch, self.CHECK = max_batch, check
        self.calls, self.codes = [], list(codes)

    def launch(self, chunk, m, ws, nbytes):
        self.calls.append((chunk, m, ws.value, nbytes))
        return self.codes.pop(0) if self.codes else 0

    def run(self, B, nbytes=64):
        self._each_chunk(B, nbytes, self.launch, "stub_forward")


@pytest.mark.parametrize("B, want", [(0, []), (1, [(0, 1)]), (2, [(0, 2)]), (5, [(0, 2), (2, 4), (4, 5)])])
def test_chunk_loop(B, want):
    op = Stub(max_batch=2)
    op.run(B, nbytes=48)
    assert [(c.start, c.stop) for c, *_ in op.calls] == want
    assert all(c.step is None and m == c.stop - c.start for c, m, *_ in op.calls)
    assert all(ws == op._ws.data_ptr() and nbytes == op._ws.numel() >= 48 for _, _, ws, nbytes in op.calls)
    assert (op._ws is None) == (B == 0)                           # nothing is allocated for an empty batch


def test_return_codes():
    assert _lib.E_ARG not in (0, 3)
    for code, error in ((_lib.E_ARG, ValueError), (3, RuntimeError)):
        op = Stub(codes=[0, code])
        with pytest.raises(error, match="^stub_forward: ") as e:
            op.run(5)
        assert type(e.value) is error and len(op.calls) == 2      # the loop stops at the chunk that failed
        op = Stub(check="check", codes=[code])
        with pytest.raises(RuntimeError, match="^stub_forward: ") as e:
            op.run(5)
        assert type(e.value) is RuntimeError and len(op.calls) == 1


def test_one_workspace_rule():
    op = Stub()
    first = op._workspace(100)
    assert first.dtype == torch.uint8 and first.numel() >= 100 and first.device.type == "cpu"
    assert op._workspace(100) is first and op._workspace(1) is first and op._workspace(99) is first
    second = op._workspace(101)
    assert second is not first and second.numel() >= 101
    smallest = second.numel()
    for nbytes in (5, 101, 100, 4096, 7, 4096, 4097, 1):
        ws = op._workspace(nbytes)
        assert ws.numel() >= max(nbytes, smallest) and ws is op._ws
        smallest = ws.numel()
    op.run(3, nbytes=16)                                          # the chunk loop takes the same tensor
    assert op._ws is ws and {c[2] for c in op.calls} == {ws.data_ptr()}


def test_taps_cut():
    flat = torch.arange(2 * 3 + 4 + 2 * 1 * 5, dtype=torch.float32)
    cut = DeviceOperator._cut(flat, [("a", (2, 3)), ("b", (4,)), ("c", (2, 1, 5))])
    assert [name for name, _ in cut] == ["a", "b", "c"]
    assert [tuple(v.shape) for _, v in cut] == [(2, 3), (4,), (2, 1, 5)]
    assert torch.equal(torch.cat([v.reshape(-1) for _, v in cut]), flat)
    assert all(v.data_ptr() == flat.data_ptr() + 4 * off for (_, v), off in zip(cut, (0, 6, 10)))      # views, in order
    for stages in ([("a", (2, 3)), ("b", (4,))], [("a", (2, 3)), ("b", (4,)), ("c", (2, 1, 5)), ("d", (1,))]):
        with pytest.raises(AssertionError):
            DeviceOperator._cut(flat, stages)


def test_taps_are_for_one_chunk():
    op = Stub(max_batch=2)
    assert tuple(op._taps_buffer(12, B=2).shape) == (12,) and op._taps_buffer(12).dtype == torch.float32
    with pytest.raises(ValueError, match="^Stub: taps are for one chunk, B = 3 > max_batch = 2$"):
        op._taps_buffer(12, B=3)


def test_cpu_path_filter():
    stages = [(name, torch.tensor(float(i))) for i, name in enumerate(
        ("conv0", "layer0.attn_probs", "layer0.attention", "logits", "layer1.attn_probs", "hidden", "attn_probs_of"))]
    kept = DeviceOperator._kept(stages, ("attn_probs", "logits"))
    assert [name for name, _ in kept] == ["conv0", "layer0.attention", "hidden", "attn_probs_of"]
    assert all(v is dict(stages)[name] for name, v in kept)
    assert DeviceOperator._kept(stages, ()) == stages

    taps, seen = [], []

    def statement(weights, x, stages_out):
        seen.append(stages_out)
        if stages_out is not None:
            stages_out += stages
        return x + 1

    op = Stub()
    assert float(op._statement(statement, torch.tensor(1.0), taps, ("hidden",))) == 2.0
    assert [name for name, _ in taps] == [name for name, _ in stages if name != "hidden"]
    assert float(op._statement(statement, torch.tensor(2.0), None, ("hidden",))) == 3.0 and seen[1] is None


def test_max_batch_refusals():
    """The texts of the operators' constructors as they were before they shared a base."""
    from instag_amd.deepspeech import DeepSpeechEncoder
    from instag_amd.hubert import HubertEncoder
    from instag_amd.parsing import FaceParser
    from instag_amd.wav2vec import Wav2Vec2CTC
    from tests import deepspeech_helpers, hubert_helpers, parsing_helpers, wav2vec_helpers
    with pytest.raises(ValueError, match="^Wav2Vec2CTC: max_batch >= 1, got 0$"):
        Wav2Vec2CTC(wav2vec_helpers.weights("S"), "cpu", max_batch=0)
    with pytest.raises(ValueError, match="^HubertEncoder: max_batch >= 1, got -2$"):
        HubertEncoder(hubert_helpers.weights("S"), "cpu", max_batch=-2)
    with pytest.raises(ValueError, match="^FaceParser: max_batch >= 1$"):
        FaceParser(parsing_helpers.weights(), "cpu", max_batch=0)
    with pytest.raises(ValueError, match="^DeepSpeechEncoder: max_rows >= 1, got 0$"):
        DeepSpeechEncoder(deepspeech_helpers.weights("A"), "cpu", max_rows=0)
    assert Wav2Vec2CTC(wav2vec_helpers.weights("S"), "cpu", max_batch=3).max_batch == 3
    assert DeepSpeechEncoder(deepspeech_helpers.weights("A"), "cpu", max_rows=5).rows_per_block(67) == 5
