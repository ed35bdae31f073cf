"""Golden G16: the project's wav2vec 2.0 statement pinned to ``transformers``, the library the reference calls.

    python tests/golden/make_golden_wav2vec.py        # writes tests/golden/g16_wav2vec.npz (CPU, needs transformers)

No weights are stored (as for G9): ``Wav2Vec2Weights.random(S, 16)``'s state dict is loaded into a
``Wav2Vec2ForCTC`` built from the matching ``Wav2Vec2Config`` -- from the config object only, nothing is fetched -- with
every dropout, layerdrop and mask probability 0, and run in fp64 on three segments of 22,400 samples.  The segments are
normalised by ``Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm``, the routine ``Wav2Vec2FeatureExtractor(
do_normalize=True)`` applies; it is called directly because the extractor's ``__call__`` casts to fp32 first, which would
leave an fp32 rounding in an fp64 golden.

Stored: the audio (fp16-exact values), the fp64 logits [3,69,44], the state dict's names and shapes, and the error of
the project's fp32 statement against these logits as measured here.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    from transformers import Wav2Vec2Config, Wav2Vec2FeatureExtractor, Wav2Vec2ForCTC

    from instag_amd.wav2vec import wav2vec2_torch
    from tests import wav2vec_helpers as H

    w = H.weights("S", H.G16_SEED)
    config = Wav2Vec2Config(**H.S.hf(), hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0,
                            feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0,
                            mask_feature_prob=0.0)
    model = Wav2Vec2ForCTC(config).double().eval()
    sd = {k: v.double() for k, v in w.state_dict().items()}
    expected = {k for k in model.state_dict() if not k.endswith("masked_spec_embed")}
    assert set(sd) == expected, set(sd) ^ expected
    if "wav2vec2.masked_spec_embed" in model.state_dict():
        sd["wav2vec2.masked_spec_embed"] = model.state_dict()["wav2vec2.masked_spec_embed"]
    model.load_state_dict(sd, strict=True)

    audio = H.seeded_audio(3, 22400, seed=H.G16_AUDIO_SEED).half()
    assert Wav2Vec2FeatureExtractor(do_normalize=True).do_normalize
    rows = [r.double().numpy() for r in audio]
    values = torch.from_numpy(np.stack(Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm(rows, None)))
    assert values.dtype == torch.float64
    with torch.no_grad():
        logits = model(input_values=values).logits
    assert tuple(logits.shape) == (3, 69, 44)
    scale = float(logits.abs().max())
    ours64 = wav2vec2_torch(w, audio.double())
    ours32 = wav2vec2_torch(w, audio.float()).double()
    e64, e32 = float((ours64 - logits).abs().max()) / scale, float((ours32 - logits).abs().max()) / scale
    print(f"max|logits| {scale:.4f}  statement fp64 {e64:.3e}  fp32 {e32:.3e}")
    names = sorted(sd)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g16_wav2vec.npz"), audio=audio.numpy(),
                        logits=logits.numpy(), names=np.array(names),
                        shapes=np.array([",".join(str(s) for s in sd[k].shape) for k in names]),
                        e32=np.float64(e32), weights_seed=np.int64(H.G16_SEED))


if __name__ == "__main__":
    main()
