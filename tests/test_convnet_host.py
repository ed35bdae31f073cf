"""Host tests of the shared network core (instag_amd/convnet.py): the one BatchNorm fold gives the bits of the three
formulas it replaced, a state dict round-trips bit for bit, and _lib.check_arg tells a refused argument from a failure.
No device is needed."""
import pytest
import torch

from instag_amd.convnet import BN_EPS


def _classes():
    from instag_amd.ave_encoder import AudioEncoderWeights
    from instag_amd.parsing import BiSeNetWeights
    from instag_amd.teeth import FPNWeights
    return dict(parsing=BiSeNetWeights, teeth=FPNWeights, ave=AudioEncoderWeights)


def _fold_before(net, lay):
    """The formula ``net``'s own ``folded`` had before the three were made one, in fp64."""
    d = {f: t.double() for f, t in lay.items()}
    n = d["weight"].shape[0]
    if net == "ave":
        scale = d["gamma"] / torch.sqrt(d["var"] + BN_EPS)
        return scale, (d["bias"] - d["mean"]) * scale + d["beta"]
    if "gamma" in d:
        scale = d["gamma"] / torch.sqrt(d["var"] + BN_EPS)
        return scale, d["beta"] - d["mean"] * scale
    ones = torch.ones(n, dtype=torch.float64)
    return ones, (torch.zeros(n, dtype=torch.float64) if net == "parsing" else d["bias"])


@pytest.mark.parametrize("seed", (0, 15))
@pytest.mark.parametrize("net", ("parsing", "teeth", "ave"))
def test_fold_and_round_trip(net, seed):
    cls = _classes()[net]
    w = cls.random(seed)
    kinds = set()
    for dtype in (torch.float64, torch.float32):
        folded = w.folded(dtype)
        assert len(folded) == len(w.layers)
        for lay, (weight, scale, shift) in zip(w.layers, folded):
            want_scale, want_shift = _fold_before(net, lay)
            assert weight.dtype == scale.dtype == shift.dtype == dtype
            assert torch.equal(weight, lay["weight"].to(dtype))
            assert torch.equal(scale, want_scale.to(dtype)) and torch.equal(shift, want_shift.to(dtype))
            kinds.add(("gamma" in lay, "bias" in lay))
    assert kinds == {"parsing": {(True, False), (False, False)}, "teeth": {(True, False), (False, True)},
                     "ave": {(True, True)}}[net]

    sd = w.state_dict()
    again = cls.from_state_dict(sd).state_dict()
    assert sd.keys() == again.keys()
    for k, v in sd.items():
        assert v.dtype == again[k].dtype and torch.equal(v, again[k]), k
    for a, b in zip(w.layers, cls.from_state_dict(sd).layers):
        assert a.keys() == b.keys() and all(torch.equal(a[f], b[f]) for f in a)


def test_check_arg():
    from instag_amd import _lib
    lib = _lib.lib()
    _lib.check_arg(0, "nothing")
    assert lib.instag_parsing_workspace_bytes(1, 64, 80) == 0                 # sets the library's error text
    text = lib.instag_last_error().decode()
    assert "multiples of 32" in text
    with pytest.raises(ValueError, match="parsing_forward: .*multiples of 32"):
        _lib.check_arg(1, "parsing_forward")                                   # INSTAG_E_ARG
    for code in (2, 3):
        with pytest.raises(RuntimeError, match="parsing_forward: .*multiples of 32") as e:
            _lib.check_arg(code, "parsing_forward")
        assert not isinstance(e.value, ValueError)
    with pytest.raises(ValueError, match="multiples of 32"):
        _lib.workspace_bytes(lib.instag_parsing_workspace_bytes(1, 64, 80))
    assert _lib.workspace_bytes(lib.instag_parsing_workspace_bytes(1, 64, 96)) > 0
