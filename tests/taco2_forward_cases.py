"""Case table of Tacotron2 with teacher forcing, shared by tools/make_golden_taco_forward.py (which runs the reference's
own ``Tacotron2.forward``) and the tests that replay the cases against the restatement (tests/taco2_forward_ref.py) and the
HIP engine.  The model shapes are those of tests/ar_cases.py.  Each case: config overrides on
parakeet_amd.synthetic.TACOTRON2_LJSPEECH, tokens T, teacher frames T_mel, seed (weights; ids, tones, global condition and
teacher = rng(850 + seed); dropout stream seed + b for utterance b), keyword arguments of synthetic.tacotron2_state, and
``output_lens`` (None: not passed to ``forward``; its length is the batch size, every utterance has T tokens)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ar_cases import T2_CASES  # noqa: E402

_SHAPE = {c[0]: c[1] for c in T2_CASES}

CASES = {
    # no stop token: nothing but mel_output / mel_outputs_postnet / alignments
    "plain": (dict(_SHAPE["nostop"]), 7, 9, 41, dict(), None),
    # tone embedding (padding id 0 included)
    "toned": (dict(_SHAPE["tones"]), 8, 6, 42, dict(stop_bias=-8.0), None),
    # stop logits of every step; p_prenet_dropout = 0.25
    "stop": (dict(_SHAPE["maxsteps"]), 9, 11, 43, dict(stop_bias=-8.0), None),
    # global condition (B, 32) concatenated to the encoder outputs (:746-751)
    "global": (dict(_SHAPE["global"]), 9, 5, 44, dict(stop_bias=-8.0), None),
    # B = 2, equal text lengths, the second utterance's output_lens shorter than T_mel: the output mask (:765-769)
    "batch2": (dict(_SHAPE["maxsteps"]), 6, 8, 45, dict(stop_bias=-8.0), (8, 5)),
}
KEYS = ("mel_output", "mel_outputs_postnet", "alignments", "stop_logits")


def case_cfg(name):
    from parakeet_amd import synthetic as syn
    return dict(syn.TACOTRON2_LJSPEECH, **CASES[name][0])


def case_state(name):
    from parakeet_amd import synthetic as syn
    _, _, _, seed, skw, _ = CASES[name]
    return syn.tacotron2_state(case_cfg(name), seed=seed, **skw)


def case_inputs(name):
    """dict(ids (B, T), tones (B, T) or None, global_condition (B, G) or None, mels (B, T_mel, d_mels), output_lens or None,
    seeds [B])."""
    _, T, L, seed, _, olens = CASES[name]
    cfg = case_cfg(name)
    B = 1 if olens is None else len(olens)
    rng = np.random.default_rng(850 + seed)
    ids = rng.integers(1, cfg["vocab_size"], size=(B, T)).astype(np.int64)
    tones = rng.integers(0, cfg["n_tones"], size=(B, T)).astype(np.int64) if cfg["n_tones"] else None
    gc = rng.standard_normal((B, cfg["d_global_condition"])).astype(np.float32) if cfg.get("d_global_condition") else None
    mels = (0.5 * rng.standard_normal((B, L, cfg["d_mels"]))).astype(np.float32)
    return dict(ids=ids, tones=tones, global_condition=gc, mels=mels,
                output_lens=None if olens is None else np.array(olens, dtype=np.int64), seeds=[seed + b for b in range(B)])
