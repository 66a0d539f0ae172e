"""Float64 numpy restatement of the evaluator criteria of FastSpeech2, TransformerTTS and Tacotron2, each kept in the
reference's own order of operations, and the derived bound of the guided-attention sums.

  FastSpeech2Loss / DurationPredictorLoss      parakeet/models/fastspeech2/fastspeech2.py:674-812,
                                               parakeet/modules/fastspeech2_predictor/duration_predictor.py:140-184
  TransformerTTSLoss, GuidedAttentionLoss,     parakeet/models/transformer_tts/transformer_tts.py:770-1082
  GuidedMultiHeadAttentionLoss
  attention_guide / guided_attention_loss      parakeet/modules/losses.py:26-57
  Tacotron2Loss                                parakeet/models/tacotron2.py:886-982
  the stop labels and lengths of forward()     transformer_tts.py:417-450

tools/make_golden_am_losses.py runs the reference's classes themselves; tests/test_am_losses_cpu.py holds this file to what
they gave.

THE BOUND OF pk_guided_attn_run (csrc/seq_loss.hip, k_guided_attn_tile), u = 2^-24.
The kernel forms, all in fp32 without contraction, ft = t / T, fs = s / S (IEEE divisions of integers below 2^24: one
rounding each, |.| <= u as both quotients are below 1; 2u each is allowed for here so that the bound also holds for a
reciprocal-multiply), d = ft - fs (u, |d| < 1): |delta d| <= 5u.  z = (d * d) / den with den = fp32(2 sigma^2), rounded once
on the host from the double sigma: the square, den and the division are three relative roundings of z.
W = 1 - expf(-z), so dW/dz = e^-z and
    |delta W| <= e^-z (|d| / sigma^2) 5u            [through d; |d| e^-z / sigma^2 is largest at |d| = sigma: 0.607 / sigma]
              +  3u z e^-z                          [z e^-z <= 1 / e = 0.368]
              +  2 ulp of expf (its result is at most 1: 2 ulp <= 4u)  +  u for the subtraction
            <=  (3.04 / sigma + 1.11 + 4 + 1) u  <=  (3.1 / sigma + 6.2) u.
Each product W * A is exact in float64 and enters a float64 accumulator (PK_SEQ_LOSS_F32_CHAIN = 0 fp32 additions); lanes,
waves and tiles are added in float64, whose roundings (n 2^-53 relative, n the entry count) vanish beside the 2u sum(WA)
the bound keeps for the conversion of the result and of the reference.  Per utterance, with the project's spare factor 2
(tests/fp32_bounds.py C_MFMA) for roundings not measured:
    bound_b = 2 [ (3.1 / sigma + 6.2) u sum(A_b) + (PK_SEQ_LOSS_F32_CHAIN + 2) u sum(W A)_b ].
"""
import numpy as np

U = 2.0 ** -24
SPARE = 2.0


# ---------------------------------------------------------------------------------------------------------------- masks
def non_pad_mask(lens, maxlen=None):
    lens = np.asarray(lens, np.int64).reshape(-1)
    maxlen = int(lens.max()) if maxlen is None else int(maxlen)
    return np.arange(maxlen)[None, :] < lens[:, None]


def _f64(x):
    return np.asarray(x, np.float64)


# -------------------------------------------------------------------------------------------------------------- guide
def guide(ilen, olen, sigma):
    """_make_guided_attention_mask (transformer_tts.py:984-989) in float64: (olen, ilen)."""
    gx, gy = np.meshgrid(np.arange(olen, dtype=np.float64), np.arange(ilen, dtype=np.float64), indexing="ij")
    return 1.0 - np.exp(-((gy / ilen - gx / olen) ** 2) / (2 * (sigma ** 2)))


def guide_f32(ilen, olen, sigma, reciprocal=False):
    """The same formula with every operation in fp32 (what the reference computes, and what the kernel computes);
    ``reciprocal``: the quotients as a multiplication by the rounded reciprocal."""
    f = np.float32
    gx, gy = np.meshgrid(np.arange(olen, dtype=f), np.arange(ilen, dtype=f), indexing="ij")
    if reciprocal:
        qy, qx = gy * (f(1) / f(ilen)), gx * (f(1) / f(olen))
    else:
        qy, qx = gy / f(ilen), gx / f(olen)
    d = (qy - qx).astype(f)
    z = ((d * d).astype(f) / f(2 * (sigma ** 2))).astype(f)
    return (f(1) - np.exp(-z).astype(f)).astype(f)


def guide_entry_bound(sigma):
    """|fp32 guide - exact guide| per entry (derivation at the top of this file)."""
    return (3.1 / sigma + 6.2) * U


def guided_sums(att, rows, cols, sigma):
    """att: (B, G, Smax, Tmax) or (B, Smax, Tmax).  -> (B, 2) float64: sum W * A and sum A over each utterance's valid
    entries of all its maps."""
    a = _f64(att)
    if a.ndim == 3:
        a = a[:, None]
    out = np.zeros((a.shape[0], 2))
    for b in range(a.shape[0]):
        S, T = int(rows[b]), int(cols[b])
        w = guide(T, S, sigma)
        v = a[b, :, :S, :T]
        out[b] = (w[None] * v).sum(), v.sum()
    return out


def guided_sums_bound(sigma, sum_a, sum_wa, chain):
    return SPARE * (guide_entry_bound(sigma) * np.abs(sum_a) + (chain + 2) * U * np.abs(sum_wa))


# ------------------------------------------------------------------------------------------------------ FastSpeech2Loss
def duration_predictor_loss(outputs, targets, offset=1.0, reduction="mean"):
    t = np.log(_f64(targets) + offset)
    e = (_f64(outputs) - t) ** 2
    return e.mean() if reduction == "mean" else e.sum() if reduction == "sum" else e


def _sel(x, mask):
    return x[np.broadcast_to(mask, x.shape)]


def fastspeech2_loss(after_outs, before_outs, d_outs, p_outs, e_outs, ys, ds, ps, es, ilens, olens, use_masking=True,
                     use_weighted_masking=False):
    assert (use_masking != use_weighted_masking) or not use_masking
    before_outs, d_outs, p_outs, e_outs = _f64(before_outs), _f64(d_outs), _f64(p_outs), _f64(e_outs)
    after_outs = None if after_outs is None else _f64(after_outs)
    ys, ds, ps, es = _f64(ys), _f64(ds), _f64(ps), _f64(es)
    if use_masking:
        om = non_pad_mask(olens)[..., None]
        before_outs = _sel(before_outs, om)
        if after_outs is not None:
            after_outs = _sel(after_outs, om)
        ys = _sel(ys, om)
        dm = non_pad_mask(ilens)
        d_outs, ds = _sel(d_outs, dm), _sel(ds, dm)
        pm = dm[..., None]
        p_outs, e_outs, ps, es = _sel(p_outs, pm), _sel(e_outs, pm), _sel(ps, pm), _sel(es, pm)
    red = "none" if use_weighted_masking else "mean"
    l1 = np.abs(before_outs - ys)
    if after_outs is not None:
        l1 = l1 + np.abs(after_outs - ys)
    dl = duration_predictor_loss(d_outs, ds, reduction=red)
    pl, el = (p_outs - ps) ** 2, (e_outs - es) ** 2
    if not use_weighted_masking:
        l1 = np.abs(before_outs - ys).mean() + (0.0 if after_outs is None else np.abs(after_outs - ys).mean())
        return l1, dl, pl.mean(), el.mean()
    om = non_pad_mask(olens)[..., None]
    ow = om.astype(np.float64) / om.astype(np.float64).sum(axis=1, keepdims=True)
    ow = ow / (ys.shape[0] * ys.shape[2])
    dm = non_pad_mask(ilens)
    dw = dm.astype(np.float64) / dm.astype(np.float64).sum(axis=1, keepdims=True)
    dw = dw / ds.shape[0]
    l1 = _sel(l1 * ow, om).sum()
    dl = _sel(dl * dw, dm).sum()
    pm, pw = dm[..., None], dw[..., None]
    return l1, dl, _sel(pl * pw, pm).sum(), _sel(el * pw, pm).sum()


# ---------------------------------------------------------------------------------------------------- TransformerTTSLoss
def bce_with_logits(x, y, pos_weight=1.0):
    """Paddle's documented binary_cross_entropy_with_logits, reduction "none":
    (1 - y) x + (1 + (pos_weight - 1) y) (log1p(exp(-|x|)) + max(-x, 0))."""
    x, y = _f64(x), _f64(y)
    return (1.0 - y) * x + (1.0 + (pos_weight - 1.0) * y) * (np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0))


def transformer_tts_loss(after_outs, before_outs, logits, ys, labels, olens, use_masking=True, use_weighted_masking=False,
                         bce_pos_weight=5.0):
    assert (use_masking != use_weighted_masking) or not use_masking
    after_outs, before_outs, logits, ys, labels = map(_f64, (after_outs, before_outs, logits, ys, labels))
    if use_masking:
        m = non_pad_mask(olens)[..., None]
        ys, after_outs, before_outs = _sel(ys, m), _sel(after_outs, m), _sel(before_outs, m)
        labels, logits = _sel(labels, m[:, :, 0]), _sel(logits, m[:, :, 0])
    bce = bce_with_logits(logits, labels, bce_pos_weight)
    if not use_weighted_masking:
        l1 = np.abs(after_outs - ys).mean() + np.abs(before_outs - ys).mean()
        l2 = ((after_outs - ys) ** 2).mean() + ((before_outs - ys) ** 2).mean()
        return l1, l2, bce.mean()
    l1 = np.abs(after_outs - ys) + np.abs(before_outs - ys)
    l2 = (after_outs - ys) ** 2 + (before_outs - ys) ** 2
    m = non_pad_mask(olens)[..., None]
    w = m.astype(np.float64) / m.sum(axis=1, keepdims=True).astype(np.float64)
    ow, lw = w / (ys.shape[0] * ys.shape[2]), w / ys.shape[0]
    return _sel(l1 * ow, m).sum(), _sel(l2 * ow, m).sum(), _sel(bce * lw[..., 0], m[..., 0]).sum()


def transformer_tts_total(l1, l2, bce, loss_type):
    """transformer_tts_updater.py:246-253."""
    if loss_type == "L1":
        return l1 + bce
    if loss_type == "L2":
        return l2 + bce
    if loss_type == "L1+L2":
        return l1 + l2 + bce
    raise ValueError("unknown --loss-type " + loss_type)


def guided_attention_loss_tts(att_ws, ilens, olens, sigma=0.4, alpha=1.0):
    """GuidedAttentionLoss.forward (3-D) and GuidedMultiHeadAttentionLoss.forward (4-D): alpha * the mean of guide * att_ws
    over the entries inside both lengths, every head counted."""
    a = _f64(att_ws)
    if a.ndim == 3:
        a = a[:, None]
    B, H, L, T = a.shape
    g = np.zeros((B, L, T))
    for b in range(B):
        g[b, :int(olens[b]), :int(ilens[b])] = guide(int(ilens[b]), int(olens[b]), sigma)
    mask = non_pad_mask(olens, L)[:, :, None] & non_pad_mask(ilens, T)[:, None, :]
    losses = g[:, None] * a
    return alpha * _sel(losses, mask[:, None]).mean()


def transformer_tts_forward_targets(text_lengths, speech_lengths, speech_frames, r=1):
    """labels, olens, ilens and the frame count of ys as forward() leaves them (transformer_tts.py:417-450)."""
    ilens = np.asarray(text_lengths, np.int64) + 1
    olens = np.asarray(speech_lengths, np.int64)
    pad = ~non_pad_mask(olens - 1)                       # make_pad_mask(olens - 1): width max(olens) - 1
    labels = np.pad(pad.astype(np.float32), ((0, 0), (0, 1)), "constant", constant_values=1.0)
    n_ys = int(speech_frames)
    if r > 1:
        olens = olens - olens % r
        max_olen = int(olens.max())
        n_ys = min(n_ys, max_olen)
        labels = labels[:, :max_olen].copy()
        labels[:, -1] = 1.0
    return labels, olens, ilens, n_ys


# ----------------------------------------------------------------------------------------------------------- Tacotron2
def attention_guide(dec_lens, enc_lens, N, T, g):
    dec_lens, enc_lens = _f64(dec_lens), _f64(enc_lens)
    dec_pos = np.arange(N, dtype=np.float64)[None, :] / dec_lens[:, None]
    enc_pos = np.arange(T, dtype=np.float64)[None, :] / enc_lens[:, None]
    W = 1 - np.exp(-(dec_pos[:, :, None] - enc_pos[:, None, :]) ** 2 / (2 * g ** 2))
    mask = non_pad_mask(dec_lens, N)[:, :, None] * non_pad_mask(enc_lens, T)[:, None, :]
    return W * mask


def guided_attention_loss(attention_weight, dec_lens, enc_lens, g):
    a = _f64(attention_weight)
    _, N, T = a.shape
    W = attention_guide(dec_lens, enc_lens, N, T, g)
    total = _f64(dec_lens) * _f64(enc_lens)
    return np.mean(np.sum(W * a, axis=(1, 2)) / total)


def tacotron2_loss(mel_outputs, mel_outputs_postnet, mel_targets, attention_weights=None, slens=None, plens=None,
                   stop_logits=None, use_stop_token_loss=True, use_guided_attention_loss=False, sigma=0.2):
    mel_loss = ((_f64(mel_outputs) - _f64(mel_targets)) ** 2).mean()
    post = ((_f64(mel_outputs_postnet) - _f64(mel_targets)) ** 2).mean()
    total = mel_loss + post
    out = {"mel_loss": mel_loss, "post_mel_loss": post}
    if use_guided_attention_loss:
        out["guided_attn_loss"] = guided_attention_loss(attention_weights, slens, plens, sigma)
        total = total + out["guided_attn_loss"]
    if use_stop_token_loss:
        T_dec = np.asarray(mel_targets).shape[1]
        labels = np.eye(T_dec)[np.asarray(slens, np.int64) - 1]
        out["stop_loss"] = bce_with_logits(stop_logits, labels).mean()
        total = total + out["stop_loss"]
    out["loss"] = total
    return out
