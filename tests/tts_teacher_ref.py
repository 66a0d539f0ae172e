"""fp64 torch restatement of TransformerTTS.inference(..., use_teacher_forcing=True) (the oracle of the teacher-forcing
tests), built from oracle/transformer_tts_ref.py's pieces.

transformer_tts.py:567-579 -> _forward :462-500: <eos> appended; encoder; + gst(ys) (the teacher spectrogram itself);
speaker integration; ys_in = ys[r - 1::r] with a zero frame in front and the last row dropped; decoder.embed once on all
L // r rows (prenet dropout as the AR decode's call at step s = L // r); every DecoderLayer without a cache under the
causal target mask (:692-723), the memory unmasked; after_norm (pre-norm blocks only); feat_out; outs = before +
postnet(before); att_ws = every layer's src_attn weights.
"""
import math

import numpy as np
import torch

from oracle import transformer_tts_ref as tt
from oracle.fastspeech2_ref import conv_ffn, postnet
from oracle.nn_ref import Weights, layer_norm, linear


def mha_masked(W, q_in, kv_in, n_head, causal):
    """MultiHeadedAttention.forward attention.py:133-156 with the causal target mask (masked_fill(min) -> softmax ->
    masked_fill(0), :118-122) or none.  Returns (output, weights (1, H, Tq, Tk))."""
    B, Tq, D = q_in.shape
    Tk = kv_in.shape[1]
    dk = D // n_head
    q = linear(q_in, W["linear_q.weight"], W["linear_q.bias"]).reshape(B, Tq, n_head, dk).transpose(1, 2)
    k = linear(kv_in, W["linear_k.weight"], W["linear_k.bias"]).reshape(B, Tk, n_head, dk).transpose(1, 2)
    v = linear(kv_in, W["linear_v.weight"], W["linear_v.bias"]).reshape(B, Tk, n_head, dk).transpose(1, 2)
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dk)
    if causal:
        keep = torch.tril(torch.ones(Tq, Tk, dtype=torch.bool))
        s = s.masked_fill(~keep, float("-inf"))
    attn = torch.softmax(s, dim=-1)
    ctx = torch.matmul(attn, v).transpose(1, 2).reshape(B, Tq, D)
    return linear(ctx, W["linear_out.weight"], W["linear_out.bias"]), attn


def decoder_layer(W, tgt, memory, n_head, normalize_before=True, concat_after=False):
    """DecoderLayer.forward decoder_layer.py:74-158 without a cache."""
    residual = tgt
    t = layer_norm(tgt, W["norm1.weight"], W["norm1.bias"]) if normalize_before else tgt
    a = mha_masked(W.sub("self_attn."), t, t, n_head, True)[0]
    x = residual + (linear(torch.cat([t, a], dim=-1), W["concat_linear1.weight"], W["concat_linear1.bias"])
                    if concat_after else a)
    if not normalize_before:
        x = layer_norm(x, W["norm1.weight"], W["norm1.bias"])
    residual = x
    h = layer_norm(x, W["norm2.weight"], W["norm2.bias"]) if normalize_before else x
    a, attn = mha_masked(W.sub("src_attn."), h, memory, n_head, False)
    x = residual + (linear(torch.cat([h, a], dim=-1), W["concat_linear2.weight"], W["concat_linear2.bias"])
                    if concat_after else a)
    if not normalize_before:
        x = layer_norm(x, W["norm2.weight"], W["norm2.bias"])
    residual = x
    h = layer_norm(x, W["norm3.weight"], W["norm3.bias"]) if normalize_before else x
    x = residual + conv_ffn(W.sub("feed_forward."), h)
    if not normalize_before:
        x = layer_norm(x, W["norm3.weight"], W["norm3.bias"])
    return x, attn[0]


def teacher_inference(state, ids, speech, cfg=None, seed=0, dropout=True, spembs=None, dtype=torch.float64):
    """ids (T,) without <eos>, speech (L, odim) -> (outs ((L // r) * r, odim), att_ws (dlayers, H, L // r, T + 1), parts)
    with parts = dict(hs, before, zs, drop_steps)."""
    cfg = dict(tt.DEFAULT_CFG, **(cfg or {}))
    r = cfg.get("reduction_factor", 1)
    W = Weights(state, dtype)
    idim = (state["encoder.embed.0.weight"] if "encoder.embed.0.weight" in state
            else state["encoder.embed.0.0.embed.weight"]).shape[0]
    odim = state["feat_out.weight"].shape[1] // r
    x = np.pad(np.asarray(ids), (0, 1), "constant", constant_values=idim - 1)
    xs = torch.as_tensor(x).to(torch.int64).unsqueeze(0)
    ys = torch.as_tensor(np.asarray(speech)).to(dtype)
    hs = tt.encode(W.sub("encoder."), xs, cfg)
    if cfg.get("use_gst"):                                                          # :475-477
        hs = hs + tt.style_encoder(W.sub("gst."), ys, cfg).unsqueeze(1)
    if cfg.get("spk_embed_dim"):                                                    # :480-481
        e = torch.as_tensor(np.asarray(spembs)).to(dtype).reshape(1, -1)
        hs = tt.integrate_with_spk_embed(W, hs, e, cfg["spk_embed_integration_type"])
    ys_in = ys[r - 1::r] if r > 1 else ys                                           # :484-489
    ys_in = torch.cat([torch.zeros(1, odim, dtype=dtype), ys_in[:-1]], dim=0).unsqueeze(0)   # :492, :661-665
    L_in = ys_in.shape[1]
    drop_steps = []
    drop = None
    if dropout and cfg["dprenet_layers"] > 0:
        stream = tt.stream_dropout(seed, cfg["dprenet_layers"], cfg["dprenet_units"])

        def drop(step, layer, rows, units):
            drop_steps.append(step)
            return stream(step, layer, rows, units)
    D = W.sub("decoder.")
    xd = tt.decoder_embed(D, ys_in, L_in, cfg, drop)
    att = []
    for l in range(cfg["dlayers"]):
        xd, a = decoder_layer(D.sub(f"decoders.{l}."), xd, hs, cfg["aheads"], cfg.get("decoder_normalize_before", True),
                              cfg.get("decoder_concat_after", False))
        att.append(a)
    zs = xd
    z = layer_norm(xd, D["after_norm.weight"], D["after_norm.bias"]) if cfg.get("decoder_normalize_before", True) else xd
    before = linear(z, W["feat_out.weight"], W["feat_out.bias"]).reshape(1, -1, odim)    # (1, L_in * r, odim)
    after = before
    if cfg["postnet_layers"] > 0:
        b = before.transpose(1, 2)
        after = (b + postnet(W.sub("postnet."), b, cfg["postnet_layers"])).transpose(1, 2)
    parts = dict(hs=hs[0], before=before[0], zs=zs[0], drop_steps=drop_steps)
    return after[0], torch.stack(att, dim=0), parts
