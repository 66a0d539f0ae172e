"""GE2E speaker encoder behind the reference's Python API.

Mirrors parakeet/models/lstm_speaker_encoder.py ``LSTMSpeakerEncoder(n_mels, num_layers, hidden_size, output_size)``
(:24-147): ``set_state_dict``, ``eval``, ``embed_sequences`` (:40-48), ``embed_utterance`` (:50-53) and the scoring side
of GE2E, forward only (no gradients): ``similarity_matrix`` (:55-104), ``loss`` (:114-147), ``inv_argmax`` (:111-112) and
``forward`` (:34-38).  The embeddings, the similarity matrix and the loss terms run in libpk_synth.so (csrc/spk.hip,
csrc/spk_loss.hip); ``similarity_weight`` / ``similarity_bias`` of a state dict are kept (10 and -5 unless given).  The
equal error rate is host code, as in the reference: ``equal_error_rate`` below, numpy only, importable without a GPU.

Extensions (supersets): ``embed_utterances`` embeds a ragged list of utterances (each a (B_u, T, n_mels) batch of
partials, one T for all) in one call; an utterance's embedding does not depend on the others of the call.
``evaluate_batch`` scores N x M partials the way a user means it (``forward`` keeps the reference's reshape),
``loss_terms`` returns the per-utterance cross-entropy terms without a host synchronisation, ``speaker_similarity`` the
cosine similarity of pairs of embeddings.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, set_params, wrap


class GE2EShapeError(ValueError, NotImplementedError):
    """An ``embeds`` shape the GE2E loss does not take: not (N, M, C), N < 2, M < 2 (the reference divides by M - 1), a
    ``forward`` reshape that does not exist, or a batch beyond the kernels' envelope.  A ValueError; it is a
    NotImplementedError too, which ``forward`` raised for every input before the loss existed, so callers that caught that
    keep working."""


def equal_error_rate(labels, scores):
    """The equal error rate the reference's ``loss`` computes (:143-145: ``roc_curve``, ``interp1d``, ``brentq``), in closed
    form and in numpy alone.

    labels: 0 / 1 (1 = target trial), scores: higher = more target-like; both are flattened.  The ROC runs over the
    DISTINCT scores in descending order (tied scores form one step) from (0, 0) to (1, 1); the result is the ``fpr`` at
    which the piecewise-linear curve meets ``tpr = 1 - fpr``.  ``tpr + fpr - 1`` rises strictly from -1 to 1 along the
    curve: the crossing is unique, found on one segment by linear interpolation; on a vertical segment it is that
    segment's ``fpr``.  Separable scores give 0, inverted ones 1, all-equal scores 0.5.  Agrees with the reference's
    pipeline to its root finder's tolerance (``brentq``'s xtol 2e-12).  ValueError without both classes or with NaN."""
    y = np.asarray(labels).reshape(-1)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if y.shape != s.shape or y.size == 0:
        raise ValueError(f"labels {np.shape(labels)} and scores {np.shape(scores)} must have the same, non-zero size")
    if np.isnan(s).any():
        raise ValueError("scores contain NaN")
    pos = y != 0
    if not np.isin(y, (0, 1)).all():
        raise ValueError("labels must be 0 or 1")
    P, Q = int(pos.sum()), int((~pos).sum())
    if P == 0 or Q == 0:
        raise ValueError("the equal error rate needs target and non-target trials")
    order = np.argsort(-s, kind="stable")
    s, pos = s[order], pos[order]
    last = np.r_[np.nonzero(s[1:] != s[:-1])[0], s.size - 1]      # the last trial of every distinct score
    tp = np.r_[0, np.cumsum(pos)[last]].astype(np.float64)
    fp = np.r_[0, np.cumsum(~pos)[last]].astype(np.float64)
    tpr, fpr = tp / P, fp / Q
    g = tpr + fpr - 1.0
    k = int(np.argmax(g >= 0.0))                                  # g[0] = -1, g[-1] = 1: 1 <= k
    if g[k] == 0.0 or fpr[k] == fpr[k - 1]:
        return float(fpr[k])
    t = -g[k - 1] / (g[k] - g[k - 1])
    return float(fpr[k - 1] + t * (fpr[k] - fpr[k - 1]))


class LSTMSpeakerEncoder:
    def __init__(self, n_mels, num_layers, hidden_size, output_size, device=None):
        self.n_mels, self.num_layers = int(n_mels), int(num_layers)
        self.hidden_size, self.output_size = int(hidden_size), int(output_size)
        self.training = True
        self._ctx = Context.get(device)
        cfg = _capi.SpkCfg(self.n_mels, self.num_layers, self.hidden_size, self.output_size)
        h = C.c_void_p()
        try:
            _capi.check(self._ctx.lib.pk_spk_create(self._ctx.handle, C.byref(cfg), C.byref(h)))
        except NotImplementedError as e:   # a size the kernels do not take is an argument error to the caller
            raise ValueError(str(e)) from e
        self._h = h
        self._finalized = False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._ctx.lib.pk_spk_destroy(h)
            except Exception:
                pass

    def set_state_dict(self, state_dict):
        set_params(self._ctx.lib.pk_spk_set_param, self._h, state_dict)
        self._finalized = False

    def eval(self):
        self.training = False
        return self

    def set_math(self, mode):
        """'f16x3' (default: split-fp16 MFMA, fp32-equivalent error) or 'f32' (exact fp32 MFMA)."""
        _capi.check(self._ctx.lib.pk_spk_set_math(self._h, {"f32": 0, "f16x3": 1}[mode]))

    def forward(self, utterances, num_speakers, initial_states=None):
        """The reference's ``forward`` (:34-38) to the letter: ``embed_sequences``, then
        ``reshape([num_speakers, -1, num_speakers])``, then ``loss`` -> (loss, eer).

        That reshape is the reference's own: the LAST axis becomes ``num_speakers``, not the embedding size, so the loss
        sees slices of embeddings (not unit-norm) -- the recipe's 64 speakers x 10 utterances x 256 dimensions arrive as
        (64, 40, 64).  It is kept as it is; ``evaluate_batch`` is the (N, M, output_size) reading.  GE2EShapeError (a
        ValueError) where B * output_size is no multiple of num_speakers^2, or the result has fewer than 2 speakers or
        2 "utterances"."""
        N = int(num_speakers)
        embeds = self.embed_sequences(utterances, initial_states)
        total = int(embeds.shape[0]) * int(embeds.shape[1])
        if N < 1 or total % (N * N) != 0:
            raise GE2EShapeError(f"forward: {tuple(embeds.shape)} embeddings do not reshape to ({N}, -1, {N})")
        return self.loss(embeds.reshape(N, -1, N))

    __call__ = forward

    # -- GE2E similarity matrix, loss, EER ---------------------------------------------------------------------------
    def _ge2e(self, embeds, sim=False, p1=False, p2=False, terms=False, loss=False):
        """pk_spk_ge2e over embeds (N, M, C) (device or host); returns the requested device tensors in a dict."""
        ctx = Context.get(self._ctx.device)
        e = ctx.to_device(embeds)
        if e.dim() != 3:
            raise GE2EShapeError(f"embeds must be (speakers, utterances, dimensions), got {tuple(e.shape)}")
        N, M, Cd = (int(v) for v in e.shape)
        if N < 2 or M < 2 or Cd < 1:
            raise GE2EShapeError(f"embeds {(N, M, Cd)}: the GE2E loss takes at least 2 speakers of at least 2 utterances "
                                 "(the exclusive centroid divides by M - 1)")
        out = {"N": N, "M": M}
        if sim:
            out["sim"] = ctx.empty((N * M, N))
        if p1:
            out["p1"] = ctx.empty((N * M * N,))
        if p2:
            out["p2"] = ctx.empty((N * M,))
        if terms:
            out["terms"] = ctx.empty((N, M), dtype=torch.float64)
        if loss:
            out["loss"] = ctx.empty((1,), dtype=torch.float64)
        ptr = lambda k: dptr(out[k]) if k in out else None   # noqa: E731
        try:
            _capi.check(ctx.lib.pk_spk_ge2e(self._h, dptr(e), N, M, Cd, ptr("sim"), ptr("p1"), ptr("p2"), ptr("terms"),
                                            ptr("loss")))
        except (NotImplementedError, AssertionError) as err:   # beyond the envelope / a refused shape
            raise GE2EShapeError(str(err)) from err
        return out

    def similarity_matrix(self, embeds):
        """embeds (N, M, C) -> (p, p1, p2) (:55-104), device tensors of shapes (N*M, N), (N*M*N,), (N*M,):
        p1 = e . normalised inclusive centroids, p2 = e . normalised exclusive centroid of its own speaker,
        p = (p1 with the own-speaker column replaced by p2) * similarity_weight + similarity_bias.
        The embeddings need not be unit-norm.  A speaker whose centroid has zero norm gives NaN, as in the reference."""
        o = self._ge2e(embeds, sim=True, p1=True, p2=True)
        return wrap(o["sim"]), wrap(o["p1"]), wrap(o["p2"])

    def inv_argmax(self, i, num):
        """One-hot row of length ``num`` with a 1 at ``i`` (:111-112; plain ``int`` for the removed ``np.int``)."""
        return np.eye(1, num, i, dtype=int)[0]

    def loss(self, embeds):
        """embeds (N, M, C) -> (loss, eer) (:114-147): the softmax GE2E loss, the mean over the N*M rows of
        logsumexp(p_row) - p_row[own speaker], as a 0-d float32 device tensor, and the equal error rate of the similarity
        matrix against the one-hot speaker labels as a Python float (``equal_error_rate`` on the host, as in the
        reference).  A speaker whose centroid has zero norm gives a NaN loss, as in the reference (and no EER: ValueError)."""
        o = self._ge2e(embeds, sim=True, loss=True)
        N, M = o["N"], o["M"]
        labels = np.zeros((N * M, N), dtype=np.int8)
        labels[np.arange(N * M), np.arange(N * M) // M] = 1
        eer = equal_error_rate(labels, o["sim"].cpu().numpy())
        return wrap(o["loss"].to(torch.float32).reshape(())), eer

    def loss_terms(self, embeds):
        """embeds (N, M, C) -> (N, M) float64 device tensor of logsumexp(p_row) - p_row[own speaker], the terms whose mean
        is the loss.  No host synchronisation, no EER."""
        return wrap(self._ge2e(embeds, terms=True)["terms"])

    def evaluate_batch(self, utterances, num_speakers, initial_states=None):
        """utterances (N * M, T, n_mels), speaker-major -> {"loss", "eer"} of
        ``embed_sequences(utterances).reshape(N, M, output_size)``: what ``forward`` would compute without its reshape."""
        N = int(num_speakers)
        embeds = self.embed_sequences(utterances, initial_states)
        if N < 1 or int(embeds.shape[0]) % N != 0:
            raise GE2EShapeError(f"evaluate_batch: {int(embeds.shape[0])} partials are no multiple of {N} speakers")
        loss, eer = self.loss(embeds.reshape(N, -1, self.output_size))
        return {"loss": loss, "eer": eer}

    def speaker_similarity(self, a, b):
        """Two (U, C) arrays of embeddings -> (U,) device tensor of cosine similarities a[u] . b[u] / (|a[u]| |b[u]|): how
        close a cloned voice is to its reference."""
        ctx = Context.get(self._ctx.device)
        x, y = ctx.to_device(a), ctx.to_device(b)
        if x.dim() != 2 or tuple(x.shape) != tuple(y.shape) or x.numel() == 0:
            raise ValueError(f"two (U, C) arrays of the same shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        out = ctx.empty((int(x.shape[0]),))
        _capi.check(ctx.lib.pk_spk_cosine(self._h, dptr(x), dptr(y), int(x.shape[0]), int(x.shape[1]), dptr(out)))
        return wrap(out)

    def _finalize(self):
        if not self._finalized:
            _capi.check(self._ctx.lib.pk_spk_finalize(self._h))
            self._finalized = True

    def _run(self, partials, initial_states, cu):
        ctx = Context.get(self._ctx.device)
        self._finalize()
        x = ctx.to_device(partials)
        if x.dim() != 3 or x.shape[2] != self.n_mels:
            raise ValueError(f"partials must be (B, T, {self.n_mels}), got {tuple(x.shape)}")
        P, T = int(x.shape[0]), int(x.shape[1])
        h0 = c0 = None
        if initial_states is not None:
            h0, c0 = (ctx.to_device(s) for s in initial_states)
            want = (self.num_layers, P, self.hidden_size)
            if tuple(h0.shape) != want or tuple(c0.shape) != want:
                raise ValueError(f"initial_states must be two {want} arrays")
        U = P if cu is None else len(cu) - 1
        out = ctx.empty((U, self.output_size))
        cu_arr = None if cu is None else np.ascontiguousarray(cu, dtype=np.int32)
        _capi.check(ctx.lib.pk_spk_embed(self._h, dptr(x), P, T, None if h0 is None else dptr(h0),
                                         None if c0 is None else dptr(c0),
                                         None if cu_arr is None else cu_arr.ctypes.data_as(C.POINTER(C.c_int32)), U,
                                         dptr(out)))
        return wrap(out)

    def embed_sequences(self, utterances, initial_states=None, reduce=False):
        """utterances (B, T, n_mels) -> (B, output_size) unit-norm embeddings; reduce=True -> (output_size,)."""
        if reduce:
            B = int(utterances.shape[0])
            return self._run(utterances, initial_states, [0, B])[0]
        return self._run(utterances, initial_states, None)

    def embed_utterance(self, utterances, initial_states=None):
        return self.embed_sequences(utterances, initial_states, reduce=True)

    def embed_utterances(self, partial_batches):
        """A list of (B_u, T, n_mels) partial batches (device or host) -> (U, output_size): embed_utterance of each,
        in one call."""
        if len(partial_batches) == 0:
            raise ValueError("no utterances")
        ctx = Context.get(self._ctx.device)
        parts = [ctx.to_device(p) for p in partial_batches]
        cu = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in parts])])
        return self._run(torch.cat(parts, 0), None, cu)
