"""Tacotron2 with teacher forcing, restated in plain torch (fp32 or fp64) for one utterance: ``Tacotron2.forward``
(parakeet/models/tacotron2.py:691-778) around ``Tacotron2Decoder.forward`` (:419-472), with eval semantics (only the
decoder prenet's dropout is live, :76-79).  Composed from the functions oracle/tacotron2_ref.py exposes; what differs
from its ``infer`` is the decoder loop: the queries are [0, mel[0], ..., mel[L - 2]] (:447-449, the last teacher frame is
never a query, :455-456), the prenet sees all of them before the loop (:451), there are exactly L steps and no stop rule.

For one utterance the masks of ``forward`` are all ones: the attention mask covers text_lens = T (:754-755), the output
mask output_lens = L (:765-769).  ``output_len`` shorter than L restates that mask: the decoder still runs L steps, rows
of mel_output / mel_outputs_postnet at or past it are zero, alignments and stop logits are not masked (:770-776).

The prenet dropout mask comes from the engine's counter-based stream, element index ((step * 2 + layer) * d_prenet +
unit): row s of the (L + 1)-row prenet call is decoding step s.  ``drop=None`` switches it off."""
import numpy as np
import torch

from oracle import tacotron2_ref as ref
from oracle.nn_ref import Weights, linear


def forward(state, ids, mel, cfg=None, tones=None, seed=0, drop="stream", dtype=torch.float32, global_condition=None,
            output_len=None, return_parts=False):
    """ids (T,) int64, mel (L, d_mels) -> dict with mel_output (L, d_mels), mel_outputs_postnet (L, d_mels),
    alignments (L, T) and, with a stop token, stop_logits (L,)."""
    cfg = dict(ref.DEFAULT_CFG, **(cfg or {}))
    if cfg.get("reduction_factor", 1) != 1:
        raise NotImplementedError("reduction_factor != 1: Tacotron2.forward cannot run it (postnet on (B, T, C * r), :762)")
    W = Weights(state, dtype)
    x = torch.as_tensor(np.asarray(ids)).to(torch.int64).reshape(1, -1)
    emb = W["embedding.weight"][x]                                                    # :739-740
    if cfg.get("n_tones"):
        tn = torch.as_tensor(np.asarray(tones)).to(torch.int64).reshape(1, -1)
        te = W["embedding_tones.weight"][tn]
        emb = emb + torch.where((tn == 0).unsqueeze(-1), torch.zeros_like(te), te)    # :741-742, padding_idx=0
    key = ref.encoder(W.sub("encoder."), emb, cfg["encoder_conv_layers"])             # :744 (text_lens = T: nothing is padded)
    enc_out = key
    if global_condition is not None:                                                  # :746-751
        g = torch.as_tensor(np.asarray(global_condition)).to(dtype).reshape(1, 1, -1)
        key = torch.cat([key, g.expand(-1, key.shape[1], -1)], dim=-1)
    D = W.sub("decoder.")
    A = D.sub("attention_layer.")
    T = key.shape[1]
    Ha, Hd = D["attention_rnn.weight_hh"].shape[1], D["decoder_rnn.weight_hh"].shape[1]
    M = cfg["d_mels"]
    teacher = torch.as_tensor(np.asarray(mel)).to(dtype).reshape(1, -1, M)
    L = teacher.shape[1]
    z = lambda n: torch.zeros(1, n, dtype=dtype)                                      # noqa: E731  (:352-372)
    att_h, att_c, dec_h, dec_c = z(Ha), z(Ha), z(Hd), z(Hd)
    attw, attw_cum, ctx = z(T), z(T), z(key.shape[2])
    pkey = linear(key, A["key_layer.weight"])                                         # :376
    p = float(cfg["p_prenet_dropout"])
    if drop == "stream":
        drop = ref.stream_dropout(seed, cfg["d_prenet"], p)
    # querys = prenet(concat([start_step, querys])) (:447-451): (1, L + 1, d_mels), row s is the query of step s
    q = torch.cat([torch.zeros(1, 1, M, dtype=dtype), teacher], dim=1)
    for j, nm in enumerate(("linear1", "linear2")):                                   # DecoderPreNet :76-79
        q = torch.relu(linear(q, D[f"prenet.{nm}.weight"]))
        if drop is not None and p > 0:
            keep = torch.as_tensor(np.stack([drop(s, j, q.shape[2]) for s in range(L + 1)]))
            q = torch.where(keep.unsqueeze(0), q / (1.0 - p), torch.zeros_like(q))
    mels, aligns, stops = [], [], []
    while len(mels) < q.shape[1] - 1:                                                 # :456, the last row is ignored
        query = q[:, len(mels), :]
        att_h, att_c = ref.lstm_cell(D.sub("attention_rnn."), torch.cat([query, ctx], dim=-1), att_h, att_c)   # :381-385
        ctx, attw = ref.location_sensitive_attention(A, att_h, pkey, key, torch.stack([attw, attw_cum], dim=-1))
        attw_cum = attw_cum + attw                                                    # :397
        dec_h, dec_c = ref.lstm_cell(D.sub("decoder_rnn."), torch.cat([att_h, ctx], dim=-1), dec_h, dec_c)   # :400-403
        hc = torch.cat([dec_h, ctx], dim=-1)
        mels.append(linear(hc, D["linear_projection.weight"], D["linear_projection.bias"]))   # :411-413
        aligns.append(attw)
        if cfg["use_stop_token"]:
            stops.append(linear(hc, D["stop_layer.weight"], D["stop_layer.bias"]))    # :415
    mel_out = torch.stack(mels, dim=1)                                                # (1, L, M)
    post = mel_out + ref.postnet(W.sub("postnet."), mel_out, cfg["postnet_conv_layers"])   # :762-763
    if output_len is not None:                                                        # :765-769
        mask = (torch.arange(L) < int(output_len)).to(dtype).reshape(1, L, 1)
        mel_out, post = mel_out * mask, post * mask
    out = dict(mel_output=mel_out[0], mel_outputs_postnet=post[0], alignments=torch.stack(aligns, dim=1)[0])
    if cfg["use_stop_token"]:
        out["stop_logits"] = torch.cat(stops, dim=1)[0]
    if return_parts:
        out["encoder_outputs"] = enc_out[0]
    return out
