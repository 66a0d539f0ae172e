"""GE2E speaker encoder behind the reference's Python API.

Mirrors parakeet/models/lstm_speaker_encoder.py ``LSTMSpeakerEncoder(n_mels, num_layers, hidden_size, output_size)``
(:24-53): ``set_state_dict``, ``eval``, ``embed_sequences`` (:40-48) and ``embed_utterance`` (:50-53).  All arithmetic
runs in libpk_synth.so (csrc/spk.hip).  Training (``forward`` / ``loss`` / ``similarity_matrix``) is out of scope;
``similarity_weight`` / ``similarity_bias`` are accepted in a state dict and ignored.

Extension (superset): ``embed_utterances`` embeds a ragged list of utterances (each a (B_u, T, n_mels) batch of
partials, one T for all) in one call; an utterance's embedding does not depend on the others of the call.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, set_params, wrap


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
        raise NotImplementedError("LSTMSpeakerEncoder.forward is the GE2E training loss; only inference is implemented")

    __call__ = forward

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
