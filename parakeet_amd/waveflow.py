"""WaveFlow vocoder behind the reference's Python API.

Mirrors parakeet/models/waveflow.py ``ConditionalWaveFlow`` (constructor :741-757, ``forward`` :759-782, ``infer``
:785-805, ``predict`` :808-825) and ``WaveFlowLoss`` (:855-891); all arithmetic of the model runs in libpk_synth.so
(csrc/waveflow.hip).  Both directions: ``infer`` samples (autoregressive over the rows of the folded signal), ``forward`` is
density estimation -- audio to the latent ``z`` and the log-determinant, hence the exact log-likelihood of a recording under the
vocoder -- and runs every row of a flow at once.  No backward pass: the engine does not train.
Extensions: ``infer`` takes an optional ``z=`` (the reference draws ``paddle.randn`` inside); ``forward_batch`` /
``log_likelihood`` take ragged lists and answer per utterance.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi, amp
from .runtime import Context, dptr, set_params, wrap

__all__ = ["ConditionalWaveFlow", "WaveFlowLoss"]

_MATH = {"f32": 0, "f16x3": 1, "f16": 2}


class WaveFlowLoss:
    """waveflow.py:855-891: the negative log-likelihood per sample of ``z`` under N(0, sigma^2) with the flow's
    log-determinant -- ``sum(z^2) / (2 sigma^2) - log_det_jacobian`` over ``prod(z.shape)`` plus ``const``."""

    def __init__(self, sigma=1.0):
        self.sigma = sigma
        self.const = 0.5 * np.log(2 * np.pi) + np.log(self.sigma)

    def forward(self, z, log_det_jacobian):
        z = z.as_subclass(torch.Tensor) if isinstance(z, torch.Tensor) else torch.as_tensor(np.asarray(z))
        ldj = log_det_jacobian
        ldj = ldj.as_subclass(torch.Tensor) if isinstance(ldj, torch.Tensor) else torch.as_tensor(np.asarray(ldj))
        loss = torch.sum(z * z) / (2 * self.sigma * self.sigma) - ldj.to(z.device)
        loss = loss / int(np.prod(z.shape))
        return wrap(loss + self.const)

    __call__ = forward


class ConditionalWaveFlow:
    def __init__(self, upsample_factors, n_flows, n_layers, n_group, channels, n_mels, kernel_size, device=None):
        if isinstance(kernel_size, int):
            kernel_size = [kernel_size, kernel_size]
        self.n_group, self.n_mels = n_group, n_mels
        self.training = True
        self._ctx = Context.get(device)
        cfg = _capi.WfCfg()
        cfg.n_upsample = len(upsample_factors)
        for i, f in enumerate(upsample_factors):
            cfg.upsample_factors[i] = int(f)
        cfg.n_flows, cfg.n_layers, cfg.n_group = n_flows, n_layers, n_group
        cfg.channels, cfg.n_mels = channels, n_mels
        cfg.kernel_h, cfg.kernel_w = int(kernel_size[0]), int(kernel_size[1])
        h = C.c_void_p()
        _capi.check(self._ctx.lib.pk_wf_create(self._ctx.handle, C.byref(cfg), C.byref(h)))
        self._h = h
        self._finalized = False
        self._math = "f16x3"
        self._last_len = None    # per utterance: length of the condition the last call kept (debug_tap)

    @classmethod
    def from_pretrained(cls, config, checkpoint_path):
        """waveflow.py:827-852: ``config`` with ``model`` / ``data`` sections (examples/waveflow/config.py; a yacs node, a
        mapping or a yaml path), ``checkpoint_path`` without the ``.pdparams`` suffix.  Like the reference it returns the
        model in training mode with the checkpoint's weight-norm pairs loaded (folded when the engine packs them): the
        recipe goes on with ``layer_tools.recursively_remove_weight_norm(model)`` and ``model.eval()``."""
        from . import checkpoint
        return checkpoint.load_waveflow(config, checkpoint_path, cls=cls, eval_mode=False)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._ctx.lib.pk_wf_destroy(h)
            except Exception:
                pass

    def set_state_dict(self, state_dict):
        set_params(self._ctx.lib.pk_wf_set_param, self._h, state_dict)
        self._finalized = False

    def eval(self):
        self.training = False
        return self

    def set_math(self, mode):
        """'f16x3' (default: split-fp16 MFMA GEMMs, fp32-equivalent error) or 'f32' (exact fp32 MFMA)."""
        _capi.check(self._ctx.lib.pk_wf_set_math(self._h, _MATH[mode]))
        self._math = mode

    def set_option(self, key, value):
        """Named integer options of the engine handle (include/pk_synth.h, pk_wf_set_option): 'layer_waves', 'fuse_step',
        'keep_cond'."""
        _capi.check(self._ctx.lib.pk_wf_set_option(self._h, key.encode(), int(value)))

    def _auto_cast(self):
        """Inside ``with parakeet_amd.amp.auto_cast():`` (examples/waveflow/synthesize.py:40) a call runs with fp16 operands --
        where the model has that mode: it lives on the fused layer kernel, and the engine answers PK_EUNSUPPORTED for every other
        model, which then runs with its own math (the reference's auto_cast works for any model).  True if the math was switched."""
        if not amp.enabled() or self._math == "f16":
            return False
        status = self._ctx.lib.pk_wf_set_math(self._h, _MATH["f16"])
        if status == _capi.PK_EUNSUPPORTED:
            return False
        _capi.check(status)
        return True

    def debug_tap(self, what, b):
        """Test tap of the last infer_batch / forward_batch: ``"cond"`` is utterance ``b``'s upsampled mel as the flows read it,
        (n_mels, T) in time order with T the length of that call's result (pk_wf_debug_read).  After an ``infer`` on the fused
        layer kernel it needs ``set_option("keep_cond", 1)`` before the call."""
        if what != "cond":
            raise ValueError(f"unknown tap {what!r}")
        known = self._last_len is not None and 0 <= b < len(self._last_len)
        n = self._last_len[b] if known else 0    # (before a call, or no such utterance: the engine refuses, whatever the size)
        out = np.empty((self.n_mels, n), dtype=np.float32)
        _capi.check(self._ctx.lib.pk_wf_debug_read(self._h, 0, int(b), _capi.fptr(out), out.size))
        return out

    def set_seed(self, seed):
        """Seed of the engine's own latent stream (``pk_randn``), used when neither ``z`` nor a torch
        ``generator`` is given -- the ``paddle.randn`` of waveflow.py:801."""
        _capi.check(self._ctx.lib.pk_wf_set_seed(self._h, int(seed) & (2 ** 64 - 1)))

    def lengths(self, t_mel):
        a, b = C.c_int32(), C.c_int32()
        _capi.check(self._ctx.lib.pk_wf_cond_length(self._h, int(t_mel), C.byref(a), C.byref(b)))
        return a.value, b.value

    def infer_batch(self, mels, zs=None, generator=None):
        """mels: list of (C_mel, T_b) arrays (ragged).  Returns a list of (T_b',) device tensors."""
        ctx = Context.get(self._ctx.device)
        if not self._finalized:
            _capi.check(ctx.lib.pk_wf_finalize(self._h))
            self._finalized = True
        frames = np.array([int(m.shape[-1]) for m in mels], dtype=np.int32)
        mel = torch.cat([ctx.to_device(m).reshape(self.n_mels, -1).transpose(0, 1) for m in mels], 0).contiguous()
        lens = [self.lengths(int(f)) for f in frames]
        total_z = sum(a for a, _ in lens)
        if zs is None:
            z = None if generator is None else torch.randn(total_z, device=ctx.device, generator=generator)
        else:
            z = torch.cat([ctx.to_device(v).reshape(-1) for v in zs])
        assert z is None or z.numel() == total_z, "z must have cond_len samples per utterance"
        wav = ctx.empty((sum(b for _, b in lens),))
        cast = self._auto_cast()
        self._last_len = [b for _, b in lens]
        try:
            _capi.check(ctx.lib.pk_wf_infer(self._h, dptr(mel), frames.ctypes.data_as(C.POINTER(C.c_int32)), len(mels),
                                            None if z is None else dptr(z), dptr(wav), 0))
        finally:
            if cast:
                _capi.check(ctx.lib.pk_wf_set_math(self._h, _MATH[self._math]))
        outs, o = [], 0
        for _, n in lens:
            outs.append(wrap(wav[o:o + n]))
            o += n
        return outs

    def forward_length(self, t_mel, n_audio):
        """Length of ``z`` for ``n_audio`` samples with ``t_mel`` frames (the audio cut to a multiple of n_group, :617-625)."""
        n = C.c_int32()
        _capi.check(self._ctx.lib.pk_wf_forward_length(self._h, int(t_mel), int(n_audio), C.byref(n)))
        return n.value

    def forward_batch(self, audios, mels):
        """Density estimation of a ragged batch.  audios: list of (T_b,) arrays, mels: list of (C_mel, T_mel_b) arrays with
        ``n_group <= T_b <= T_mel_b * hop`` (the untrimmed upsampled mel must cover the audio, waveflow.py:618, 780).
        Returns a list of ``(z_b, logdet_b)``: z_b (T_b // n_group * n_group,) fp32 device tensor, logdet_b a 0-d fp64 device
        tensor (the sum of logs of utterance b).  An utterance's results do not depend on the rest of the batch."""
        ctx = Context.get(self._ctx.device)
        if not self._finalized:
            _capi.check(ctx.lib.pk_wf_finalize(self._h))
            self._finalized = True
        assert len(audios) == len(mels) and len(mels) > 0
        frames = np.array([int(m.shape[-1]) for m in mels], dtype=np.int32)
        auds = [ctx.to_device(a).reshape(-1) for a in audios]
        alen = np.array([int(a.numel()) for a in auds], dtype=np.int32)
        zlen = [self.forward_length(int(f), int(n)) for f, n in zip(frames, alen)]   # raises ValueError on a bad length
        mel = torch.cat([ctx.to_device(m).reshape(self.n_mels, -1).transpose(0, 1) for m in mels], 0).contiguous()
        audio = torch.cat(auds).contiguous()
        z = ctx.empty((sum(zlen),))
        logdet = ctx.empty((len(mels),), dtype=torch.float64)
        cast = self._auto_cast()
        self._last_len = list(zlen)
        try:
            i32p = C.POINTER(C.c_int32)
            _capi.check(ctx.lib.pk_wf_forward(self._h, dptr(mel), frames.ctypes.data_as(i32p), dptr(audio), alen.ctypes.data_as(i32p),
                                              len(mels), dptr(z), dptr(logdet), 0))
        finally:
            if cast:
                _capi.check(ctx.lib.pk_wf_set_math(self._h, _MATH[self._math]))
        outs, o = [], 0
        for b, n in enumerate(zlen):
            outs.append((wrap(z[o:o + n]), wrap(logdet[b])))
            o += n
        return outs

    def forward(self, audio, mel):
        """audio (B, T), mel (B, C_mel, T_mel) -> (z (B, T // n_group * n_group), log_det_jacobian (1,) fp32: the sum over the
        batch); waveflow.py:759-782."""
        ctx = Context.get(self._ctx.device)
        audio, mel = ctx.to_device(audio), ctx.to_device(mel)
        if not self._finalized:     # (before the length check: a call before the weights are set is a state error first)
            _capi.check(ctx.lib.pk_wf_finalize(self._h))
            self._finalized = True
        outs = self.forward_batch([audio[b] for b in range(mel.shape[0])], [mel[b] for b in range(mel.shape[0])])
        z = torch.stack([o.as_subclass(torch.Tensor) for o, _ in outs], 0)
        ldj = torch.stack([l.as_subclass(torch.Tensor) for _, l in outs]).sum().to(torch.float32).reshape(1)
        return wrap(z), wrap(ldj)

    __call__ = forward

    def log_likelihood(self, audios, mels, sigma=1.0):
        """Mean log-likelihood in nats per sample of each utterance (ragged lists as forward_batch): minus WaveFlowLoss(sigma) of
        that utterance alone.  Returns a list of floats."""
        const = 0.5 * np.log(2 * np.pi) + np.log(sigma)
        out = []
        for z, ld in self.forward_batch(audios, mels):
            zz = z.as_subclass(torch.Tensor).double()
            nll = (float(torch.sum(zz * zz)) / (2 * sigma * sigma) - float(ld)) / zz.numel() + const
            out.append(-nll)
        return out

    def infer(self, mel, z=None):
        """(B, C_mel, T_mel) -> (B, T); waveflow.py:785-805."""
        ctx = Context.get(self._ctx.device)
        mel = ctx.to_device(mel)
        zs = None if z is None else [ctx.to_device(z)[b] for b in range(mel.shape[0])]
        outs = self.infer_batch([mel[b] for b in range(mel.shape[0])], zs)
        return wrap(torch.stack([o.as_subclass(torch.Tensor) for o in outs], 0))

    def predict(self, mel, z=None):
        """np (C_mel, T_mel) -> np (T,); waveflow.py:808-825."""
        z = None if z is None else np.asarray(z)[None]
        return self.infer(np.asarray(mel)[None], z)[0].numpy()
