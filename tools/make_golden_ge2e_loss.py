#!/usr/bin/env python
"""tests/golden/ge2e_loss.npz: the REFERENCE's own GE2E similarity matrix, loss and EER on fixed embeddings.

Runs parakeet/models/lstm_speaker_encoder.py (LSTMSpeakerEncoder.similarity_matrix :55-104, loss :114-147, forward
:34-38) over oracle/paddle_shim, with the REAL sklearn (roc_curve) and scipy (interp1d, brentq) -- unlike
tools/make_golden_ge2e.py, which stubs them.  The stand-in lacks some of what these lines call; the missing pieces are
attached to the imported stand-in at run time, in this process only (nothing under oracle/ changes).  Their semantics
are read from Paddle's API documentation, like the rest of the stand-in, and are stated next to each one below.

The embeddings are handed over as float64 tensors: the stand-in (torch) then carries float64 through every line, so the
goldens pin the fp64 restatement tests/ge2e_loss_ref.py to 1e-12.  The case through ``forward`` runs embed_sequences in
the stand-in's float32 and is recorded twice: ``forward``'s own float32 loss and EER, and ``loss`` of the same
(float32-valued) embeddings under the literal reshape in float64.  Weights are not stored: they are
``parakeet_amd.synthetic.ge2e_state(cfg, seed)``.
Needs the reference checkout.  Run from the repository root:  python tools/make_golden_ge2e_loss.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402
import ge2e_loss_ref  # noqa: E402

SECOND = dict(n_mels=80, num_layers=2, hidden_size=128, output_size=64)
# name, (N, M, C), seed, unit rows, similarity_weight, similarity_bias (None: the constructor's 10 and -5)
CASES = [("a", (4, 3, 8), 1, True, None, None),
         ("b", (6, 4, 32), 2, True, None, None),
         ("wb", (5, 3, 16), 3, False, 7.5, -2.0)]
FORWARD = dict(num_speakers=4, partials=8, frames=12, seed=31, x_seed=6)


def _attach(paddle, nn):
    """What lstm_speaker_encoder.py:29-134 calls and the stand-in does not have."""
    if not hasattr(np, "int"):
        np.int = int   # :112 uses the alias numpy 2 removed
    if not hasattr(nn.Layer, "create_parameter"):
        # Layer.create_parameter(shape, default_initializer=...): a float32 parameter filled by the initializer
        nn.Layer.create_parameter = lambda self, shape, dtype="float32", default_initializer=None, **k: \
            paddle.create_parameter(shape, dtype, default_initializer=default_initializer)
    w = paddle._wrap
    if not hasattr(paddle, "mean"):
        # paddle.mean(x, axis, keepdim): arithmetic mean over the axis
        paddle.mean = lambda x, axis=None, keepdim=False, name=None: \
            w(torch.mean(x) if axis is None else torch.mean(x, dim=axis, keepdim=keepdim))
    if not hasattr(paddle, "norm"):
        # paddle.norm(x, p=2, axis, keepdim): the vector p-norm over the axis, (sum |x|^p)^(1/p)
        paddle.norm = lambda x, p=2, axis=None, keepdim=False, name=None: \
            w(torch.linalg.vector_norm(x, ord=p, dim=axis, keepdim=keepdim))
    if not hasattr(paddle, "broadcast_to"):
        # paddle.broadcast_to(x, shape): numpy broadcasting to the given shape
        paddle.broadcast_to = lambda x, shape, name=None: w(torch.broadcast_to(x, tuple(int(s) for s in shape)))
    if not hasattr(paddle, "bmm"):
        # paddle.bmm(x, y): (b, n, m) x (b, m, p) -> (b, n, p), one matrix product per batch entry
        paddle.bmm = lambda x, y, name=None: w(torch.bmm(x, y))
    if not hasattr(paddle, "scatter"):
        # paddle.scatter(x, index, updates, overwrite=True): a copy of x with rows x[index[i]] = updates[i] (the indices
        # here are distinct, so the overwrite / accumulate distinction does not arise).  Paddle wants equal dtypes; the
        # result here takes the wider of the two so that float64 embeddings stay float64 through the float32 `ones`.
        def scatter(x, index, updates, overwrite=True, name=None):
            out = x.clone().to(torch.result_type(x, updates))
            out[index.to(torch.int64)] = updates.to(out.dtype)
            return w(out)
        paddle.scatter = scatter
    if not hasattr(nn, "CrossEntropyLoss"):
        # nn.CrossEntropyLoss()(input (R, K) logits, label (R,) int64): softmax over the last axis, -log of the label's
        # probability, mean over the R rows (reduction='mean', soft_label=False, no weight)
        class CrossEntropyLoss(nn.Layer):
            def forward(self, input, label):   # noqa: A002
                lse = torch.logsumexp(input, dim=-1)
                own = torch.gather(input, -1, label.to(torch.int64).reshape(-1, 1)).reshape(-1)
                return w(torch.mean(lse - own))
        nn.CrossEntropyLoss = CrossEntropyLoss


def _np(t):
    return np.asarray(t.numpy() if hasattr(t, "numpy") else t)


def main():
    ref_import.setup()
    import paddle
    from paddle import nn
    _attach(paddle, nn)
    import scipy
    import sklearn
    from parakeet_amd import synthetic as syn
    spec = importlib.util.spec_from_file_location(
        "ref_lstm_speaker_encoder_loss", os.path.join(ref_import.REF, "parakeet", "models", "lstm_speaker_encoder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {"case_names": np.array([c[0] for c in CASES] + ["fwd"])}
    model = mod.LSTMSpeakerEncoder(SECOND["n_mels"], SECOND["num_layers"], SECOND["hidden_size"], SECOND["output_size"])
    model.set_state_dict(syn.ge2e_state(SECOND, seed=FORWARD["seed"]))
    model.eval()

    def record(name, embeds64):
        with paddle.no_grad():
            p, p1, p2 = model.similarity_matrix(paddle.to_tensor(embeds64))
            loss, eer = model.loss(paddle.to_tensor(embeds64))
        assert _np(p).dtype == np.float64 and _np(loss).dtype == np.float64
        out[f"{name}_p"], out[f"{name}_p1"], out[f"{name}_p2"] = _np(p), _np(p1), _np(p2)
        out[f"{name}_loss"] = np.float64(_np(loss))
        out[f"{name}_eer"] = np.float64(eer)

    for name, shape, seed, unit, sw, sb in CASES:
        e = ge2e_loss_ref.embeddings(*shape, seed=seed, normalise=unit)
        with torch.no_grad():
            model.similarity_weight.fill_(10.0 if sw is None else sw)
            model.similarity_bias.fill_(-5.0 if sb is None else sb)
        out[f"{name}_embeds"] = e
        out[f"{name}_wb"] = np.array([_np(model.similarity_weight)[0], _np(model.similarity_bias)[0]], np.float32)
        record(name, e.astype(np.float64))
    with torch.no_grad():
        model.similarity_weight.fill_(10.0)
        model.similarity_bias.fill_(-5.0)
    # forward(:34-38): the stand-in's float32 embed_sequences, the literal reshape, loss
    F = FORWARD
    x = np.exp(np.random.default_rng(F["x_seed"]).normal(-2.0, 2.0, size=(F["partials"], F["frames"], SECOND["n_mels"])))
    x = x.astype(np.float32)
    with paddle.no_grad():
        loss32, eer32 = model.forward(paddle.to_tensor(x), F["num_speakers"])
        seqs = _np(model.embed_sequences(paddle.to_tensor(x))).astype(np.float32)
    N = F["num_speakers"]
    out["fwd_seed"] = np.array(F["seed"])
    out["fwd_num_speakers"] = np.array(N)
    out["fwd_x"] = x
    out["fwd_seqs"] = seqs
    out["fwd_forward_loss32"] = np.float32(_np(loss32))
    out["fwd_forward_eer32"] = np.float64(eer32)
    out["fwd_embeds"] = seqs.reshape(N, -1, N)
    out["fwd_wb"] = np.array([10.0, -5.0], np.float32)
    record("fwd", out["fwd_embeds"].astype(np.float64))
    out["versions"] = np.array([f"sklearn {sklearn.__version__}", f"scipy {scipy.__version__}"])
    path = os.path.join(ref_import.golden_dir(), "ge2e_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
