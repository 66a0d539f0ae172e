"""FastSpeech2 with given durations, pitch and energy, restated in plain torch (fp32 or fp64) for one utterance:
``FastSpeech2._forward(xs, ilens, olens, ds, ps, es, is_inference=False)`` (parakeet/models/fastspeech2/fastspeech2.py
:377-466), which ``forward`` (:286-375) and ``inference(use_teacher_forcing=True)`` (:531-544) reach.  Composed from the
functions oracle/fastspeech2_ref.py exposes; what differs from its ``inference`` is the variance adaptor: the duration
predictor's log-domain output (``DurationPredictor.forward``, duration_predictor.py:85-103), the embeddings of the GIVEN
pitch and energy, the length regulator on the GIVEN durations without alpha (:433-442)."""
import numpy as np
import torch

from oracle import fastspeech2_ref as ref
from oracle.nn_ref import Weights, conv1d, linear, make_non_pad_mask, make_pad_mask


def forward(state, ids, ds, ps, es, cfg=None, dtype=torch.float32, spk_id=None, spembs=None):
    """ids, ds (T,) int64; ps, es (T,) -> dict(before (L, odim), after, d_outs (T,), p_outs (T,), e_outs (T,)) with
    L = reduction_factor * sum(ds)."""
    cfg = dict(ref.DEFAULT_CFG, **(cfg or {}))
    W = Weights(state, dtype)
    x = torch.as_tensor(np.asarray(ids)).to(torch.int64)
    ilens = [int(x.shape[0])]
    x_masks = make_non_pad_mask(ilens).unsqueeze(-2)
    hs = ref.encoder(W.sub("encoder."), x.unsqueeze(0), x_masks, cfg["elayers"], cfg["aheads"], True,
                     cfg.get("encoder_normalize_before", True), cfg.get("encoder_concat_after", False))      # :393
    if cfg.get("spk_embed_dim") is not None:                                                                 # :396-402
        emb = None
        if spembs is not None:
            emb = torch.as_tensor(np.asarray(spembs)).to(dtype).reshape(1, -1)
        elif spk_id is not None:
            emb = W["spk_embedding_table.weight"][int(spk_id)].reshape(1, -1)
            if int(spk_id) == 0:
                emb = torch.zeros_like(emb)
        if emb is not None:
            hs = ref.integrate_spk_embed(W, hs, emb, cfg.get("spk_embed_integration_type", "add"))
    d_masks = make_pad_mask(ilens)                                                                           # :410
    p_outs = ref.variance_predictor(W.sub("pitch_predictor."), hs, d_masks, cfg["pitch_predictor_layers"])
    e_outs = ref.variance_predictor(W.sub("energy_predictor."), hs, d_masks, cfg["energy_predictor_layers"])
    # DurationPredictor.forward: the same conv stack and Linear(chans -> 1), squeezed and masked, nothing else (:434)
    Wd = W.sub("duration_predictor.")
    d_outs = linear(ref.conv_relu_ln_stack(Wd, hs.transpose(1, 2), cfg["duration_predictor_layers"]).transpose(1, 2),
                    Wd["linear.weight"], Wd["linear.bias"]).squeeze(-1)
    d_outs = torch.where(d_masks, torch.zeros_like(d_outs), d_outs)
    pt = torch.as_tensor(np.asarray(ps)).to(dtype).reshape(1, -1, 1)
    et = torch.as_tensor(np.asarray(es)).to(dtype).reshape(1, -1, 1)
    kp, ke = W["pitch_embed.0.weight"].shape[-1], W["energy_embed.0.weight"].shape[-1]
    p_embs = conv1d(pt.transpose(1, 2), W["pitch_embed.0.weight"], W["pitch_embed.0.bias"],
                    padding=(kp - 1) // 2).transpose(1, 2)                                                   # :436-437
    e_embs = conv1d(et.transpose(1, 2), W["energy_embed.0.weight"], W["energy_embed.0.bias"],
                    padding=(ke - 1) // 2).transpose(1, 2)                                                   # :438-439
    hs2 = hs + e_embs + p_embs                                                                               # :440
    dt = torch.as_tensor(np.asarray(ds)).to(torch.int64).reshape(1, -1)
    odim_r = W["feat_out.weight"].shape[-1]
    r = cfg.get("reduction_factor", 1)
    odim = odim_r // r
    if int(dt.sum()) == 0:
        z = torch.zeros((0, odim), dtype=dtype)
        return dict(before=z, after=z, d_outs=d_outs[0], p_outs=p_outs[0, :, 0], e_outs=e_outs[0, :, 0])
    hs_up = ref.length_regulate(hs2, dt)                                                                     # :442
    # h_masks covers olens // r = sum(ds) rows (:445-452): every row of a single utterance, i.e. no mask
    zs = ref.encoder(W.sub("decoder."), hs_up, None, cfg["dlayers"], cfg["aheads"], False,
                     cfg.get("decoder_normalize_before", True), cfg.get("decoder_concat_after", False))      # :455
    before = linear(zs, W["feat_out.weight"], W["feat_out.bias"]).reshape(1, -1, odim)                       # :457
    after = before
    if cfg["postnet_layers"] > 0:
        after = before + ref.postnet(W.sub("postnet."), before.transpose(1, 2), cfg["postnet_layers"]).transpose(1, 2)
    return dict(before=before[0], after=after[0], d_outs=d_outs[0], p_outs=p_outs[0, :, 0], e_outs=e_outs[0, :, 0])
