"""SpeedySpeech on the HIP engine -- same class names and call conventions as
parakeet/models/speedyspeech/speedyspeech.py (SpeedySpeech :142-218, SpeedySpeechInference :221-231).

Extensions (supersets): ``inference_batch`` for ragged batches, and ``same_padding_resets_dilation`` (see
include/pk_synth.h, pk_ss_cfg): True (default) reproduces Paddle's conv kernels, which ignore the dilation
under padding="same"; False computes the dilated convolutions as the source is written.

With given durations (``SpeedySpeech.forward`` :166-184) there are two readings.  ``forward`` is the reference's: a
(B, T) rectangle without masks, in which a short utterance's convolutions see its padding tokens (id 0 embeds to zero, but
ReLU(prenet bias) is not zero) and its decoder sees the frames between its own length and the batch's, zero rows plus the
positional encoding.  ``teacher_forced_batch`` is the ragged one: every utterance as if it were alone, which is ``forward``
at B = 1 and what ground-truth-aligned mels want.  ``evaluate_batch`` / ``evaluate_per_utterance`` are the numbers of
SpeedySpeechEvaluator.evaluate_core (speedyspeech_updater.py:110-157) under the two readings."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, set_params, to_numpy_f32, wrap


def _ids(v):
    return np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v).astype(np.int64).reshape(-1)


def _host2d(v):
    return np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v).astype(np.int64)


def _losses(l1_sum, l1_n, map_sum, map_n, dur_sum, dur_n):
    """evaluate_core's means and their sum (:126-142) in float64 from the device's sums."""
    l1 = float(np.float64(l1_sum) / l1_n)
    ssim_loss = float(1.0 - np.float64(map_sum) / map_n)
    dur = float(np.float64(dur_sum) / dur_n)
    return {"l1_loss": l1, "ssim_loss": ssim_loss, "duration_loss": dur, "loss": l1 + ssim_loss + dur}


class SpeedySpeech:
    def __init__(self, vocab_size, encoder_hidden_size, encoder_kernel_size, encoder_dilations,
                 duration_predictor_hidden_size, decoder_hidden_size, decoder_output_size, decoder_kernel_size,
                 decoder_dilations, tone_size=None, same_padding_resets_dilation=True, device=None):
        self._ctx = Context.get(device)
        self.odim = decoder_output_size
        self._hidden = encoder_hidden_size
        self.training = True
        cfg = _capi.SsCfg()
        cfg.vocab_size = vocab_size
        cfg.tone_size = int(tone_size or 0)
        cfg.encoder_hidden_size, cfg.encoder_kernel_size = encoder_hidden_size, encoder_kernel_size
        cfg.duration_predictor_hidden_size = duration_predictor_hidden_size
        cfg.decoder_hidden_size, cfg.decoder_output_size = decoder_hidden_size, decoder_output_size
        cfg.decoder_kernel_size = decoder_kernel_size
        if len(encoder_dilations) > 32 or len(decoder_dilations) > 32:
            raise NotImplementedError("at most 32 residual blocks per stack")
        cfg.n_encoder_dilations, cfg.n_decoder_dilations = len(encoder_dilations), len(decoder_dilations)
        for i, d in enumerate(encoder_dilations):
            cfg.encoder_dilations[i] = int(d)
        for i, d in enumerate(decoder_dilations):
            cfg.decoder_dilations[i] = int(d)
        cfg.same_padding_resets_dilation = 1 if same_padding_resets_dilation else 0
        h = C.c_void_p()
        _capi.check(self._ctx.lib.pk_ss_create(self._ctx.handle, C.byref(cfg), C.byref(h)))
        self._h = h
        self._finalized = False
        self._last_tok, self._last_frames = [], []

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._ctx.lib.pk_ss_destroy(h)
            except Exception:
                pass

    def set_state_dict(self, state_dict):
        set_params(self._ctx.lib.pk_ss_set_param, self._h, state_dict)
        self._finalized = False

    def eval(self):
        self.training = False
        return self

    def set_normalizer(self, normalizer):
        """Register ZScore statistics; applied only by calls passing ``denormalize=True`` (see FastSpeech2)."""
        self._norm_owner = None
        if normalizer is None:
            _capi.check(self._ctx.lib.pk_ss_set_normalizer(self._h, None, None, 0))
        else:
            mu, sigma = to_numpy_f32(normalizer.mu).reshape(-1), to_numpy_f32(normalizer.sigma).reshape(-1)
            _capi.check(self._ctx.lib.pk_ss_set_normalizer(self._h, _capi.fptr(mu), _capi.fptr(sigma), mu.size))
        self._finalized = False

    def set_math(self, mode):
        """'f16x3' (default: split-fp16 MFMA GEMMs, fp32-equivalent error) or 'f32' (exact fp32 MFMA)."""
        _capi.check(self._ctx.lib.pk_ss_set_math(self._h, {"f32": 0, "f16x3": 1}[mode]))

    def _finalize(self):
        if not self._finalized:
            _capi.check(self._ctx.lib.pk_ss_finalize(self._h))
            self._finalized = True

    def encode_batch(self, texts, tones=None):
        ctx = Context.get(self._ctx.device)
        self._finalize()
        ids = [_ids(t) for t in texts]
        lens = np.array([len(i) for i in ids], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(ids))
        tflat = None
        if tones is not None:
            tn = [_ids(t) for t in tones]
            assert [len(t) for t in tn] == [len(i) for i in ids], "one tone per phone"
            tflat = np.ascontiguousarray(np.concatenate(tn))
        frames = np.zeros(len(ids), dtype=np.int32)
        i64p = C.POINTER(C.c_int64)
        _capi.check(ctx.lib.pk_ss_encode(self._h, flat.ctypes.data_as(i64p),
                                         None if tflat is None else tflat.ctypes.data_as(i64p),
                                         lens.ctypes.data_as(C.POINTER(C.c_int32)), len(ids),
                                         frames.ctypes.data_as(C.POINTER(C.c_int32))))
        self._last_tok, self._last_frames = [int(v) for v in lens], [int(v) for v in frames]
        return frames

    def decode_packed(self, denormalize=False):
        ctx = Context.get(self._ctx.device)
        total = int(sum(self._last_frames))
        mel = ctx.empty((total, self.odim))
        if total:
            _capi.check(ctx.lib.pk_ss_decode(self._h, dptr(mel), _capi.PK_APPLY_NORMALIZER if denormalize else 0))
        return mel

    def inference_batch(self, texts, tones=None, denormalize=False):
        """Lists of (T_b,) phone / tone ids -> list of (L_b, output_size) device tensors."""
        frames = self.encode_batch(texts, tones)
        mel = self.decode_packed(denormalize)
        outs, o = [], 0
        for f in frames:
            outs.append(wrap(mel[o:o + int(f)]))
            o += int(f)
        return outs

    def inference(self, text, tones=None, denormalize=False):
        """(T,) int -> (L, output_size); speedyspeech.py:178-218."""
        return self.inference_batch([text], None if tones is None else [tones], denormalize)[0]

    # ---- given durations ----------------------------------------------------------------------------------------------
    def _encode_given(self, ids, tones, durs, frame_lens):
        ctx = Context.get(self._ctx.device)
        self._finalize()
        for b, (i, d) in enumerate(zip(ids, durs)):
            if len(i) != len(d):
                raise ValueError(f"utterance {b}: {len(i)} tokens, {len(d)} durations")
        lens = np.array([len(i) for i in ids], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(ids))
        dflat = np.ascontiguousarray(np.concatenate(durs))
        tflat = None
        if tones is not None:
            if [len(t) for t in tones] != [len(i) for i in ids]:
                raise ValueError("one tone per phone")
            tflat = np.ascontiguousarray(np.concatenate(tones))
        frames = np.zeros(len(ids), dtype=np.int32)
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        fl = None if frame_lens is None else np.ascontiguousarray(frame_lens, dtype=np.int32)
        _capi.check(ctx.lib.pk_ss_encode_given(self._h, flat.ctypes.data_as(i64p),
                                               None if tflat is None else tflat.ctypes.data_as(i64p),
                                               lens.ctypes.data_as(i32p), dflat.ctypes.data_as(i64p),
                                               None if fl is None else fl.ctypes.data_as(i32p), len(ids),
                                               frames.ctypes.data_as(i32p)))
        self._last_tok, self._last_frames = [int(v) for v in lens], [int(v) for v in frames]
        return frames

    def _pred_durations(self):
        ctx = Context.get(self._ctx.device)
        out = ctx.empty((int(sum(self._last_tok)),))
        _capi.check(ctx.lib.pk_ss_pred_durations(self._h, dptr(out), 0))
        return out

    def _duration_loss_sums(self, n_valid=None):
        ctx = Context.get(self._ctx.device)
        B = len(self._last_tok)
        if n_valid is not None:
            nv = np.ascontiguousarray(n_valid, dtype=np.int32).reshape(-1)
            _capi.check(ctx.lib.pk_ss_set_valid_tokens(self._h, nv.ctypes.data_as(C.POINTER(C.c_int32)), nv.size))
        out = ctx.empty((B,), dtype=torch.float64)
        _capi.check(ctx.lib.pk_ss_duration_loss(self._h, dptr(out), 0))
        return out.cpu().numpy()

    def _split(self, packed, sizes):
        outs, o = [], 0
        for n in sizes:
            outs.append(wrap(packed[o:o + int(n)]))
            o += int(n)
        return outs

    def teacher_forced_batch(self, texts, durations, tones=None, denormalize=False, return_pred_durations=False):
        """Lists of (T_b,) phone ids, durations (frames per phone, >= 0) and tone ids -> list of (sum(d_b), output_size)
        device tensors: ``forward`` (:166-184) of every utterance as if it were alone, in one encode and one decode.  With
        ``return_pred_durations`` also the list of (T_b,) log-durations the duration predictor gave."""
        if durations is None:
            raise ValueError("teacher forcing needs durations")
        ids, durs = [_ids(t) for t in texts], [_ids(d) for d in durations]
        if len(ids) != len(durs):
            raise ValueError(f"{len(ids)} texts, {len(durs)} duration arrays")
        frames = self._encode_given(ids, None if tones is None else [_ids(t) for t in tones], durs, None)
        mels = self._split(self.decode_packed(denormalize), frames)
        if not return_pred_durations:
            return mels
        return mels, self._split(self._pred_durations(), self._last_tok)

    @staticmethod
    def _rect(text, tones, durations):
        tx, ds = _host2d(text), _host2d(durations)
        tn = None if tones is None else _host2d(tones)
        if tx.ndim != 2 or ds.shape != tx.shape or (tn is not None and tn.shape != tx.shape):
            raise ValueError(f"text {tx.shape}, tones {None if tn is None else tn.shape} and durations {ds.shape} must be "
                             "one (B, T) shape")
        return tx, tn, ds

    def forward(self, text, tones, durations):
        """speedyspeech.py:166-184: (B, T) ints -> ``(decoded (B, t_dec, output_size), pred_durations (B, T))``, t_dec the
        largest sum of durations.  The reference's rectangle: no masks, so the padding of a short utterance reaches its last
        valid tokens and frames through the convolutions, and its frames past sum(d_b) hold the decoder's answer to zero
        rows plus the positional encoding."""
        tx, tn, ds = self._rect(text, tones, durations)
        B, T = tx.shape
        t_dec = int(ds.sum(1).max()) if ds.size else 0
        if (ds < 0).any():
            raise ValueError("negative duration")
        self._encode_given([tx[b] for b in range(B)], None if tn is None else [tn[b] for b in range(B)],
                           [ds[b] for b in range(B)], [t_dec] * B)
        decoded = self.decode_packed(False).reshape(B, t_dec, self.odim)
        return wrap(decoded), wrap(self._pred_durations().reshape(B, T))

    __call__ = forward

    def evaluate_batch(self, text, tones, durations, feats, num_frames, num_phones):
        """SpeedySpeechEvaluator.evaluate_core (speedyspeech_updater.py:110-157) on one padded batch: ``forward``, then
        ``{"l1_loss", "ssim_loss", "duration_loss", "loss"}`` as Python floats.  The device leaves sums (pk_mel_loss_run,
        pk_ss_duration_loss); the means are formed here in float64: sum |decoded - feats| over the valid frames /
        (sum(num_frames) * output_size), 1 - sum of the SSIM map / (B * t_dec * output_size), the Huber sum over the valid
        tokens / sum(num_phones)."""
        from .losses import mel_loss_sums
        tx, tn, ds = self._rect(text, tones, durations)
        B, T = tx.shape
        nf, nph = _ids(num_frames), _ids(num_phones)
        if nf.size != B or nph.size != B:
            raise ValueError(f"num_frames ({nf.size}) and num_phones ({nph.size}) need one entry per utterance ({B})")
        decoded, _ = self.forward(tx, tn, ds)
        t_dec = decoded.shape[1]
        ctx = Context.get(self._ctx.device)
        tgt = ctx.to_device(feats)
        if tuple(tgt.shape) != (B, t_dec, self.odim):
            raise ValueError(f"feats {tuple(tgt.shape)}, the batch decodes to {(B, t_dec, self.odim)}")
        if (nf < 0).any() or (nf > t_dec).any() or (nph < 0).any() or (nph > T).any() or nf.sum() == 0 or nph.sum() == 0:
            raise ValueError("num_frames must lie in [0, t_dec] and num_phones in [0, T], and neither may be all zero")
        # pk_mel_loss_run takes the valid rows packed; the rows past num_frames[b] are the mask's zeros
        pack = lambda x: torch.cat([x[b, :int(nf[b])] for b in range(B)])   # noqa: E731
        sums = mel_loss_sums(pack(decoded.as_subclass(torch.Tensor)), pack(tgt), nf, padded=[t_dec] * B)
        dsum = self._duration_loss_sums(nph)
        return _losses(sums[:, 0].sum(), float(nf.sum()) * self.odim, sums[:, 1].sum(), float(B) * t_dec * self.odim,
                       dsum.sum(), float(nph.sum()))

    def evaluate_per_utterance(self, texts, durations, target_mels, tones=None):
        """The evaluator's four numbers of every utterance taken alone (B = 1: no padding, every frame and token valid) ->
        list of dicts.  One ragged encode, decode and loss pass; an utterance's numbers are the same bits in any batch.  A
        target whose length is not its utterance's sum of durations raises ValueError."""
        from .losses import mel_loss_sums
        ctx = Context.get(self._ctx.device)
        durs = [_ids(d) for d in durations]
        tgts = [ctx.to_device(t) for t in target_mels]
        if len(tgts) != len(durs):
            raise ValueError(f"{len(durs)} utterances, {len(tgts)} target mels")
        for b, (d, t) in enumerate(zip(durs, tgts)):
            if t.dim() != 2 or t.shape[1] != self.odim or t.shape[0] != int(d.sum()):
                raise ValueError(f"pair {b}: target mel {tuple(t.shape)}, the durations sum to {int(d.sum())} frames of "
                                 f"{self.odim} bins")
            if int(d.sum()) == 0:
                raise ValueError(f"pair {b}: the durations sum to no frame, there is nothing to average")
        ids = [_ids(t) for t in texts]
        frames = self._encode_given(ids, None if tones is None else [_ids(t) for t in tones], durs, None)
        packed = self.decode_packed(False)
        sums = mel_loss_sums(packed, torch.cat(tgts) if len(tgts) > 1 else tgts[0], frames)
        dsum = self._duration_loss_sums()
        return [_losses(sums[b, 0], float(frames[b]) * self.odim, sums[b, 1], float(frames[b]) * self.odim, dsum[b],
                        float(self._last_tok[b])) for b in range(len(ids))]

    def debug_tap(self, what, b):
        T = self._last_tok[b]
        out = np.empty((T, self._hidden) if what == 0 else (T,), dtype=np.float32)
        _capi.check(self._ctx.lib.pk_ss_debug_read(self._h, what, b, _capi.fptr(out), out.size))
        return out


class SpeedySpeechInference:
    """SpeedySpeechInference (speedyspeech.py:221-231): inference then normalizer.inverse."""

    def __init__(self, normalizer, speedyspeech_model):
        self.normalizer = normalizer
        self.acoustic_model = speedyspeech_model
        self.bind()

    def bind(self):
        m = self.acoustic_model
        if getattr(m, "_norm_owner", None) is not self:
            m.set_normalizer(self.normalizer)
            m._norm_owner = self
        return m

    def forward(self, phones, tones=None):
        return self.bind().inference(phones, tones, denormalize=True)

    __call__ = forward

    def eval(self):
        return self
