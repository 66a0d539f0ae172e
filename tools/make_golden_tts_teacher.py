#!/usr/bin/env python
"""Golden vectors of TransformerTTS.inference(..., use_teacher_forcing=True) from the REFERENCE's own Python source
(parakeet/models/transformer_tts/transformer_tts.py :567-579 -> _forward :462-500) executed over the torch-backed paddle
stand-in, for every case of tests/ar_cases.py TTS_CASES.  Build container only.

The teacher spectrogram of a case is standard_normal((L, 80)) of rng(1200 + seed) with L = 3 T + 1 frames (T tokens), one
more where that would be a multiple of reduction_factor r > 1: L is never a multiple of r for the r = 2 and r = 3 cases.  Prenet dropout stays on; the hook is make_golden_ar's
TransformerTTSDropout unchanged: the teacher-forced decoder calls the prenet once per layer on all L // r rows, so its
step is that row count (recorded as <case>_drop_rows).

Two things the stand-in needs that the reference uses on this branch: ``paddle.logical_and`` (``_target_mask`` :723) is
supplied here at run time, and for r > 1 ``olens.new(...)`` (:486) is a torch idiom the stand-in's Tensor accepts (real
Paddle's Tensor has no ``.new``); the vectors are what the stand-in computes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

ref_import.setup()
import paddle  # noqa: E402  (stand-in or real, see ref_import)

from make_golden_ar import TTS_CASES, TransformerTTSDropout  # noqa: E402
from parakeet_amd import synthetic as syn  # noqa: E402

OUT = ref_import.golden_dir()


def teacher_frames(T, r):
    L = 3 * T + 1
    return L + 1 if r > 1 and L % r == 0 else L


def teacher_speech(T, r, seed):
    return np.random.default_rng(1200 + seed).standard_normal((teacher_frames(T, r), 80)).astype(np.float32)


class RecordingDropout(TransformerTTSDropout):
    """TransformerTTSDropout that also records the row count of every call."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.rows = []

    def __call__(self, shape, p):
        self.rows.append(shape[1])
        return super().__call__(shape, p)


def ensure_logical_and():
    if not hasattr(paddle, "logical_and"):
        import torch
        paddle.logical_and = lambda x, y: paddle.to_tensor(torch.logical_and(torch.as_tensor(x), torch.as_tensor(y)))


def main():
    ensure_logical_and()
    ttm = ref_import.load("parakeet.models.transformer_tts.transformer_tts")
    out = {}
    for name, over, idim, T, seed, skw, kw in TTS_CASES:
        cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, **over)
        state = syn.transformer_tts_state(idim, 80, cfg, seed=seed, **skw)
        model = ttm.TransformerTTS(idim=idim, odim=80, **cfg)
        model.set_state_dict(state)
        model.eval()
        ids = syn.phoneme_ids(T, idim=idim, seed=700 + seed)
        spemb = None
        if cfg.get("spk_embed_dim"):
            spemb = np.random.default_rng(900 + seed).standard_normal(cfg["spk_embed_dim"]).astype(np.float32)
            out[f"{name}_spemb"] = spemb
        speech = teacher_speech(T, cfg.get("reduction_factor", 1), seed)
        hook = RecordingDropout(seed=seed, n_layers=max(cfg["dprenet_layers"], 1), units=cfg["dprenet_units"])
        with ref_import.dropout_hook(hook), paddle.no_grad():
            mel, probs, att = model.inference(paddle.to_tensor(ids), spembs=None if spemb is None else paddle.to_tensor(spemb),
                                              speech=paddle.to_tensor(speech), use_teacher_forcing=True)
        assert probs is None
        out[f"{name}_ids"] = ids
        out[f"{name}_seed"] = np.array(seed)
        out[f"{name}_speech"] = speech
        out[f"{name}_mel"] = mel.numpy().astype(np.float32)
        out[f"{name}_att"] = att.numpy().astype(np.float32)
        out[f"{name}_drop_rows"] = np.array(hook.rows, dtype=np.int64)
        print("transformer_tts teacher", name, out[f"{name}_mel"].shape, out[f"{name}_att"].shape, "dropout rows", hook.rows)
    np.savez_compressed(os.path.join(OUT, "tts_teacher.npz"), **out)


if __name__ == "__main__":
    main()
