"""Generate golden G9 (tests/golden/g9_ave_encoder.npz): the reference's AudioEncoder (scene/motion_net.py:102-129) in
fp64 on the windows of a seeded mel.

Run in the build container only (needs the reference checkout; never on the GPU box), on the CPU:

    python tests/golden/make_golden_ave_encoder.py

The reference's scene/motion_net.py is imported the way make_golden_ave.py does it (the oracle grid encoder injected as
`gridencoder`, the CUDA extensions never imported).  No weights are stored: the seeded rule of
tests/ave_encoder_helpers.py is loaded through the reference's own key mapping (scene/dataset_readers.py:118).  The
windows are cut by a transcription of AudDataset (utils/audio_utils.py:120-155; the module itself imports librosa at
its top and cannot be imported here).  Stored: the mel [40, 80] as fp16, the fp64 outputs [9, 512], the window starts,
every block's fraction of positive units, and the state-dict names and shapes.
"""
import sys
sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree
import importlib.util
import json
import os
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _reference_motion_net():
    sys.path.insert(0, ROOT)
    from oracle import grid_torch
    fake = types.ModuleType("gridencoder")
    fake.GridEncoder = grid_torch.GridEncoder
    sys.modules["gridencoder"] = fake
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("ref_motion_net_ave_encoder", f"{REF}/scene/motion_net.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.path.remove(REF)
    return mod


def ave_encoder():
    mn = _reference_motion_net()
    from tests import ave_encoder_helpers as H
    model = mn.AudioEncoder().eval()
    ckpt = H.state_dict()
    model.load_state_dict({f'audio_encoder.{k}': v for k, v in ckpt.items()})      # dataset_readers.py:118
    model = model.double()
    layout = sorted((k, list(v.shape)) for k, v in ckpt.items())

    mel = H.seeded_mel(H.G9_T)
    res = dict(mel=mel.numpy().astype(np.float16))
    assert np.array_equal(res["mel"].astype(np.float32), mel.numpy())
    starts = H.reference_starts(H.G9_T)
    assert starts == [0, 3, 6, 9, 12, 16, 19, 22, 24]                              # the last window is the clamped one
    windows = H.reference_windows(mel).double()
    taps = []
    hooks = [blk.register_forward_hook(lambda m, i, o: taps.append(o.detach())) for blk in model.audio_encoder]
    with torch.no_grad():
        out = model(windows)
    for h in hooks:
        h.remove()
    assert out.dtype == torch.float64 and tuple(out.shape) == (9, 512) and len(taps) == 13
    positive = H.liveness(taps)
    assert all(0.25 <= p <= 0.75 for p in positive), positive                      # every layer is alive on both sides
    assert float((out == 0).double().mean()) > 0.05 and float((out > 0).double().mean()) > 0.05
    res.update(out=out.numpy(), starts=np.asarray(starts, dtype=np.int32), positive=np.asarray(positive),
               layout=np.frombuffer(json.dumps(layout).encode(), dtype=np.uint8))
    path = f"{HERE}/g9_ave_encoder.npz"
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("positive fraction per layer", [round(p, 3) for p in positive], "max |out|", float(out.abs().max()))
    with torch.no_grad():
        out32 = model.float()(windows.float()).double()
    print("fp32 torch vs fp64: max abs", float((out32 - out).abs().max()),
          "relative to max |out|", float((out32 - out).abs().max() / out.abs().max()))


if __name__ == "__main__":
    ave_encoder()
