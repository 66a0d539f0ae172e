#!/usr/bin/env python
"""Golden values of the acoustic models' criteria from the REFERENCE's own classes -- FastSpeech2Loss,
DurationPredictorLoss, TransformerTTSLoss, GuidedAttentionLoss, GuidedMultiHeadAttentionLoss, Tacotron2Loss,
guided_attention_loss, attention_guide -- executed over the torch-backed paddle stand-in on the seeded inputs of
tests/am_loss_cases.py.  Writes tests/golden/am_losses.npz: float32 results only (the inputs are regenerated from their
seeds).  Build container only.

What the stand-in lacks is supplied here, in this process, before the reference's modules are imported: the criteria
``nn.L1Loss`` / ``nn.MSELoss`` with a reduction, ``nn.BCEWithLogitsLoss``, ``paddle.meshgrid`` / ``mean`` / ``logical_and``,
``F.one_hot`` and ``paddle.fluid.layers.sequence_mask`` (``Tensor.masked_select`` / ``broadcast_to`` come with torch).
BCE with a pos_weight follows Paddle's documentation of ``paddle.nn.functional.binary_cross_entropy_with_logits``:
    log_weight = (pos_weight - 1) * label + 1
    loss = (1 - label) * logit + log_weight * (log(1 + exp(-|logit|)) + max(-logit, 0)),
then the reduction.  Everything runs in float32, as the reference does."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import ref_import  # noqa: E402

ref_import.setup()
import paddle  # noqa: E402

import am_loss_cases as cases  # noqa: E402


def _supply():
    import paddle.fluid.layers as FL
    import paddle.nn.functional as PF
    import torch

    T = lambda x: torch.as_tensor(x).as_subclass(torch.Tensor)   # noqa: E731

    def reduce(x, reduction):
        return paddle.to_tensor(x.mean() if reduction == "mean" else x.sum() if reduction == "sum" else x)

    class _Criterion(paddle.nn.Layer):
        def __init__(self, reduction="mean", **kw):
            super().__init__()
            self.reduction = reduction

    class L1Loss(_Criterion):
        def forward(self, input, label):   # noqa: A002  (Paddle's argument name)
            return reduce(torch.abs(T(input) - T(label)), self.reduction)

    class MSELoss(_Criterion):
        def forward(self, input, label):   # noqa: A002
            return reduce((T(input) - T(label)) ** 2, self.reduction)

    class BCEWithLogitsLoss(_Criterion):
        def __init__(self, weight=None, reduction="mean", pos_weight=None, name=None):
            super().__init__(reduction)
            assert weight is None
            self.pos_weight = pos_weight

        def forward(self, logit, label):
            x, y = T(logit), T(label).to(torch.float32)
            sp = torch.log1p(torch.exp(-torch.abs(x))) + torch.clamp(-x, min=0.0)
            lw = 1.0 if self.pos_weight is None else (T(self.pos_weight) - 1.0) * y + 1.0
            return reduce((1.0 - y) * x + lw * sp, self.reduction)

    paddle.nn.L1Loss, paddle.nn.MSELoss, paddle.nn.BCEWithLogitsLoss = L1Loss, MSELoss, BCEWithLogitsLoss
    if not hasattr(paddle, "meshgrid"):
        paddle.meshgrid = lambda *xs: [paddle.to_tensor(g) for g in torch.meshgrid(*[T(x) for x in xs], indexing="ij")]
    if not hasattr(paddle, "mean"):
        paddle.mean = lambda x, axis=None, keepdim=False: paddle.to_tensor(
            torch.mean(T(x)) if axis is None else torch.mean(T(x), dim=axis, keepdim=keepdim))
    if not hasattr(paddle, "logical_and"):
        paddle.logical_and = lambda x, y: paddle.to_tensor(torch.logical_and(T(x), T(y)))
    if not hasattr(PF, "one_hot"):
        PF.one_hot = lambda x, num_classes: paddle.to_tensor(
            torch.nn.functional.one_hot(T(x).to(torch.int64), num_classes).to(torch.float32))

    def sequence_mask(x, maxlen=None, dtype="int64", name=None):
        x = T(x).to(torch.int64)
        maxlen = int(x.max()) if maxlen is None else int(maxlen)
        return paddle.cast(paddle.to_tensor(torch.arange(maxlen)[None, :] < x[:, None]), dtype)

    FL.sequence_mask = sequence_mask


def main():
    if not ref_import.REAL:
        _supply()
    fs2 = ref_import.load("parakeet.models.fastspeech2.fastspeech2")
    dp = ref_import.load("parakeet.modules.fastspeech2_predictor.duration_predictor")
    ttm = ref_import.load("parakeet.models.transformer_tts.transformer_tts")
    taco = ref_import.load("parakeet.models.tacotron2")
    losses = ref_import.load("parakeet.modules.losses")
    pt = paddle.to_tensor
    f32 = lambda t: np.asarray(t.numpy() if hasattr(t, "numpy") else t, np.float32)   # noqa: E731
    out = {}
    with paddle.no_grad():
        x = cases.fs2_inputs()
        for name, (um, uw, with_after) in cases.FS2_CASES.items():
            kw = {k: pt(v) for k, v in x.items()}
            if not with_after:
                kw["after_outs"] = None
            out[name] = np.stack([f32(v) for v in fs2.FastSpeech2Loss(use_masking=um, use_weighted_masking=uw)(**kw)])
        for name, (offset, seed) in cases.DUR_CASES.items():
            o, t = cases.dur_inputs(seed)
            out[name] = f32(dp.DurationPredictorLoss(offset=offset)(pt(o), pt(t)))
        x = cases.tts_inputs()
        for name, (um, uw, pw) in cases.TTS_CASES.items():
            l1, l2, bce = ttm.TransformerTTSLoss(use_masking=um, use_weighted_masking=uw, bce_pos_weight=pw)(
                **{k: pt(v) for k, v in x.items()})
            out[name] = np.stack([f32(l1), f32(l2), f32(bce)])
            # the evaluator's totals (transformer_tts_updater.py:246-251), formed from the reference's tensors
            out[name + "_totals"] = np.stack([f32(l1 + bce), f32(l2 + bce), f32(l1 + l2 + bce)])
        for name, (cls, sigma, alpha, heads) in cases.GA_CASES.items():
            att = cases.attention(31, heads)
            crit = getattr(ttm, cls)(sigma=sigma, alpha=alpha)
            out[name] = f32(crit(pt(att), pt(cases.ILENS), pt(cases.OLENS)))
        for name, (ilen, olen, sigma) in cases.TABLES.items():
            out[name] = f32(ttm.GuidedAttentionLoss._make_guided_attention_mask(ilen, olen, sigma))
        x = cases.taco_inputs()
        for name, (stop, guided, sigma) in cases.TACO_CASES.items():
            d = taco.Tacotron2Loss(use_stop_token_loss=stop, use_guided_attention_loss=guided, sigma=sigma)(
                **{k: pt(v) for k, v in x.items()})
            for k, v in d.items():
                out[f"{name}/{k}"] = f32(v)
        att = x["attention_weights"]
        out["guided_attention_loss"] = f32(losses.guided_attention_loss(pt(att), pt(cases.OLENS), pt(cases.ILENS), cases.GUIDE_G))
        out["attention_guide"] = f32(losses.attention_guide(pt(cases.OLENS), pt(cases.ILENS), att.shape[1], att.shape[2],
                                                           cases.GUIDE_G, paddle.float32))
    for k, v in out.items():
        print(k, v.shape, v.reshape(-1)[:4], flush=True)
    np.savez_compressed(os.path.join(ref_import.golden_dir(), "am_losses.npz"), **out)


if __name__ == "__main__":
    main()
