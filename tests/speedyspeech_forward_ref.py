"""``SpeedySpeech.forward(text, tones, durations)`` (parakeet/models/speedyspeech/speedyspeech.py:166-184) composed from the
blocks of oracle/speedyspeech_ref.py, in any dtype.  TEST INFRASTRUCTURE ONLY.

``forward`` is the reference's rectangle: (B, T) ids without masks, ``expand`` (modules/expansion.py:19-37) to the batch's
longest sum of durations, the positional encoding on every frame.  ``forward_single`` is one utterance alone, B = 1: the
ragged reading of ``teacher_forced_batch``.  ``golden_batch`` is the batch of tests/golden/speedyspeech_forward.npz."""
import numpy as np
import torch

from oracle import speedyspeech_ref as ssr
from oracle.nn_ref import Weights

VOCAB, TONES, STATE_SEED = 70, 7, 303
TOKENS = (5, 9, 14)


def golden_batch():
    """(text, tones, durations) (3, 14) int64, padded with zeros, (num_phones, num_frames), and the seeded target (3, t_dec, 80)
    float32.  Durations come from 0..6 with zeros among them; utterance 1 is one frame longer than utterance 0."""
    g = np.random.default_rng(20211)
    T = max(TOKENS)
    text, tones, durs = (np.zeros((3, T), np.int64) for _ in range(3))
    for b, n in enumerate(TOKENS):
        text[b, :n] = g.integers(1, VOCAB, n)
        tones[b, :n] = g.integers(1, TONES, n)
        durs[b, :n] = g.integers(0, 7, n)
    durs[0, 1] = 0
    durs[2, 13] = 0
    durs[1, 0] += durs[0].sum() + 1 - durs[1].sum() if durs[1].sum() <= durs[0].sum() else 0
    while durs[1].sum() > durs[0].sum() + 1:                 # trim utterance 1 down to one frame more than utterance 0
        j = int(np.argmax(durs[1]))
        durs[1, j] -= 1
    assert durs[1].sum() == durs[0].sum() + 1 and durs.min() == 0 and durs.max() <= 6
    frames = durs.sum(1)
    feats = g.standard_normal((3, int(frames.max()), 80)).astype(np.float32)
    return text, tones, durs, np.array(TOKENS, np.int64), frames.astype(np.int64), feats


def expand(enc, durations):
    """modules/expansion.py:19-37 as a gather: (B, T, C), (B, T) -> (B, max_b sum(d), C), zero rows past sum(d_b)."""
    B, T, Cn = enc.shape
    durations = np.asarray(durations)
    t_dec = int(durations.sum(1).max())
    out = torch.zeros(B, t_dec, Cn, dtype=enc.dtype)
    for b in range(B):
        rows = [j for j in range(T) for _ in range(int(durations[b, j]))]
        if rows:
            out[b, :len(rows)] = enc[b, rows]
    return out


def forward(state, text, tones, durations, cfg=None, dtype=torch.float32, same_padding_resets_dilation=True):
    """(B, T) ints -> (decoded (B, t_dec, odim), pred_durations (B, T)) as numpy."""
    from parakeet_amd.synthetic import SPEEDYSPEECH_BAKER
    cfg = dict(SPEEDYSPEECH_BAKER, **(cfg or {}))
    rd = same_padding_resets_dilation
    W = Weights(state, dtype)
    tx = torch.as_tensor(np.asarray(text)).to(torch.int64)
    tn = None if tones is None else torch.as_tensor(np.asarray(tones)).to(torch.int64)
    enc = ssr.encoder(W.sub("encoder."), tx, tn, cfg["encoder_dilations"], rd)
    pred = ssr.duration_predictor(W.sub("duration_predictor."), enc, rd)
    x = expand(enc, durations)
    x = x + ssr.sinusoid_position_encoding(x.shape[1], x.shape[2], dtype)
    out = ssr.decoder(W.sub("decoder."), x, cfg["decoder_dilations"], rd)
    return out.numpy(), pred.numpy()


def forward_single(state, text, tones, durations, **kw):
    """One utterance alone -> (decoded (sum(d), odim), pred_durations (T,))."""
    dec, pred = forward(state, np.asarray(text)[None], None if tones is None else np.asarray(tones)[None],
                        np.asarray(durations)[None], **kw)
    return dec[0], pred[0]
