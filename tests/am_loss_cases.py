"""Seeded inputs of the acoustic models' criteria (FastSpeech2Loss, TransformerTTSLoss, the guided attention losses,
Tacotron2Loss) shared by tools/make_golden_am_losses.py, tests/test_am_losses_cpu.py and tests/test_am_losses_gpu.py.
Everything is float32 / int64 numpy; padded regions hold values too (so that a criterion that forgets its mask shows)."""
import numpy as np

ODIM = 5
# ragged lengths; utterance 1 has a single token and a single frame
ILENS = np.array([7, 1, 4], np.int64)
OLENS = np.array([19, 1, 11], np.int64)

# name -> (use_masking, use_weighted_masking, with after_outs)
FS2_CASES = {
    "fs2_mask": (True, False, True),
    "fs2_none": (False, False, True),
    "fs2_weighted": (False, True, True),
    "fs2_mask_noafter": (True, False, False),
    "fs2_weighted_noafter": (False, True, False),
}
# name -> (offset, seed)
DUR_CASES = {"dur_1": (1.0, 11), "dur_half": (0.5, 12)}
# name -> (use_masking, use_weighted_masking, bce_pos_weight)
TTS_CASES = {
    "tts_mask_pw5": (True, False, 5.0),
    "tts_mask_pw1": (True, False, 1.0),
    "tts_none_pw5": (False, False, 5.0),
    "tts_none_pw1": (False, False, 1.0),
    "tts_weighted_pw5": (False, True, 5.0),
    "tts_weighted_pw1": (False, True, 1.0),
}
LOSS_TYPES = ("L1", "L2", "L1+L2")
# name -> (class, sigma, alpha, heads)
GA_CASES = {
    "ga_s04": ("GuidedAttentionLoss", 0.4, 1.0, 0),
    "ga_s02_a3": ("GuidedAttentionLoss", 0.2, 3.0, 0),
    "gmha_s04": ("GuidedMultiHeadAttentionLoss", 0.4, 1.0, 3),
    "gmha_s10_a05": ("GuidedMultiHeadAttentionLoss", 1.0, 0.5, 4),
}
# name -> (use_stop_token_loss, use_guided_attention_loss, sigma)
TACO_CASES = {
    "taco_stop": (True, False, 0.2),
    "taco_none": (False, False, 0.2),
    "taco_guided": (False, True, 0.2),
    "taco_both": (True, True, 0.4),
}
# (ilen, olen, sigma) of the two tables in GuidedAttentionLoss._make_guided_attention_mask's docstring
TABLES = {"table_5_5": (5, 5, 0.4), "table_3_6": (3, 6, 0.4)}
# GuidedAttentionLoss._make_guided_attention_mask's docstring (transformer_tts.py:963-981), as printed
TABLE_5_5 = [[0.0000, 0.1175, 0.3935, 0.6753, 0.8647],
             [0.1175, 0.0000, 0.1175, 0.3935, 0.6753],
             [0.3935, 0.1175, 0.0000, 0.1175, 0.3935],
             [0.6753, 0.3935, 0.1175, 0.0000, 0.1175],
             [0.8647, 0.6753, 0.3935, 0.1175, 0.0000]]
TABLE_3_6 = [[0.0000, 0.2934, 0.7506],
             [0.0831, 0.0831, 0.5422],
             [0.2934, 0.0000, 0.2934],
             [0.5422, 0.0831, 0.0831],
             [0.7506, 0.2934, 0.0000],
             [0.8858, 0.5422, 0.0831]]
GUIDE_G = 0.2   # attention_guide's case: dec_lens = OLENS, enc_lens = ILENS


def _f32(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def fs2_inputs(seed=21):
    """The eleven arguments of FastSpeech2Loss.forward as a dict (after_outs included)."""
    rng = np.random.default_rng(seed)
    B, L, T = len(ILENS), int(OLENS.max()), int(ILENS.max())
    return {
        "after_outs": _f32(rng, B, L, ODIM), "before_outs": _f32(rng, B, L, ODIM),
        "d_outs": _f32(rng, B, T), "p_outs": _f32(rng, B, T, 1), "e_outs": _f32(rng, B, T, 1),
        "ys": _f32(rng, B, L, ODIM), "ds": rng.integers(0, 9, (B, T)).astype(np.int64),
        "ps": _f32(rng, B, T, 1), "es": _f32(rng, B, T, 1), "ilens": ILENS.copy(), "olens": OLENS.copy(),
    }


def dur_inputs(seed):
    rng = np.random.default_rng(seed)
    return _f32(rng, 3, 9), rng.integers(0, 12, (3, 9)).astype(np.int64)


def tts_inputs(seed=22):
    """after_outs, before_outs, logits, ys, labels, olens of TransformerTTSLoss.forward; the labels are forward()'s: 1 at the
    last frame and in the padding.  Two logits are large (+-30): the stable form must carry them."""
    rng = np.random.default_rng(seed)
    B, L = len(OLENS), int(OLENS.max())
    logits = _f32(rng, B, L, scale=3.0)
    logits[0, 3], logits[2, 5] = 30.0, -30.0
    labels = (np.arange(L)[None, :] >= (OLENS[:, None] - 1)).astype(np.float32)
    return {"after_outs": _f32(rng, B, L, ODIM), "before_outs": _f32(rng, B, L, ODIM), "logits": logits,
            "ys": _f32(rng, B, L, ODIM), "labels": labels, "olens": OLENS.copy()}


def attention(seed, heads=0, ilens=ILENS, olens=OLENS):
    """Row-softmax attention over each utterance's valid columns, zero in the padding: (B, Lmax, Tmax), or
    (B, heads, Lmax, Tmax) with heads > 0."""
    rng = np.random.default_rng(seed)
    B, L, T = len(ilens), int(max(olens)), int(max(ilens))
    H = max(heads, 1)
    a = np.zeros((B, H, L, T), np.float64)
    for b in range(B):
        z = rng.standard_normal((H, int(olens[b]), int(ilens[b])))
        e = np.exp(z - z.max(-1, keepdims=True))
        a[b, :, :int(olens[b]), :int(ilens[b])] = e / e.sum(-1, keepdims=True)
    a = a.astype(np.float32)
    return a if heads > 0 else a[:, 0]


def taco_inputs(seed=23):
    """mel_outputs, mel_outputs_postnet, mel_targets, attention_weights, slens, plens, stop_logits of Tacotron2Loss."""
    rng = np.random.default_rng(seed)
    B, L = len(OLENS), int(OLENS.max())
    return {"mel_outputs": _f32(rng, B, L, ODIM), "mel_outputs_postnet": _f32(rng, B, L, ODIM),
            "mel_targets": _f32(rng, B, L, ODIM), "attention_weights": attention(seed + 100), "slens": OLENS.copy(),
            "plens": ILENS.copy(), "stop_logits": _f32(rng, B, L, scale=3.0)}
