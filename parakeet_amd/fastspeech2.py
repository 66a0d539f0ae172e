"""FastSpeech2 acoustic model behind the reference's Python API.

Mirrors parakeet/models/fastspeech2/fastspeech2.py: ``FastSpeech2`` (constructor
kwargs :52-118, ``set_state_dict``, ``eval``, ``inference`` :468-558) and
``FastSpeech2Inference`` (:662-671).  All arithmetic runs in libpk_synth.so
(csrc/fs2.hip on the transformer machinery of csrc/fft.hip, csrc/gemm.hip).
``forward`` (:286-375) and ``inference(use_teacher_forcing=True)`` run ``_forward(..., ds, ps, es,
is_inference=False)`` (:433-442) with given durations, pitch and energy.  ``FastSpeech2Loss`` (:674-812) and
``DurationPredictorLoss`` (modules/fastspeech2_predictor/duration_predictor.py:140-184) reduce on the engine
(``pk_pair_loss_run``); ``evaluate_batch`` is ``FastSpeech2Evaluator.evaluate_core``.  No gradients.

Extensions over the reference: ``inference_batch`` runs a ragged batch in one engine call (the
reference's ``inference`` is one utterance per call), ``teacher_forced_batch`` does the same with given
targets, ``predict_batch`` returns the predicted durations / pitch / energy without decoding, and
``inference_batch(durations=, pitch=, energy=)`` synthesises with edited ones (prosody control).
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, set_params, to_numpy_f32, wrap


def _host(x):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)


class FastSpeech2:
    def __init__(self, idim, odim, adim=384, aheads=4, elayers=6, eunits=1536, dlayers=6, dunits=1536,
                 postnet_layers=5, postnet_chans=512, postnet_filts=5, positionwise_layer_type="conv1d",
                 positionwise_conv_kernel_size=1, use_scaled_pos_enc=True, use_batch_norm=True,
                 encoder_normalize_before=True, decoder_normalize_before=True, encoder_concat_after=False,
                 decoder_concat_after=False, reduction_factor=1, encoder_type="transformer",
                 decoder_type="transformer", duration_predictor_layers=2, duration_predictor_chans=384,
                 duration_predictor_kernel_size=3, energy_predictor_layers=2, energy_predictor_chans=384,
                 energy_predictor_kernel_size=3, energy_predictor_dropout=0.5, energy_embed_kernel_size=9,
                 energy_embed_dropout=0.5, stop_gradient_from_energy_predictor=False,
                 pitch_predictor_layers=2, pitch_predictor_chans=384, pitch_predictor_kernel_size=3,
                 pitch_predictor_dropout=0.5, pitch_embed_kernel_size=9, pitch_embed_dropout=0.5,
                 stop_gradient_from_pitch_predictor=False, num_speakers=None, spk_embed_dim=None,
                 spk_embed_integration_type="add", num_tones=None, tone_embed_dim=None,
                 tone_embed_integration_type="add", transformer_enc_dropout_rate=0.1,
                 transformer_enc_positional_dropout_rate=0.1, transformer_enc_attn_dropout_rate=0.1,
                 transformer_dec_dropout_rate=0.1, transformer_dec_positional_dropout_rate=0.1,
                 transformer_dec_attn_dropout_rate=0.1, duration_predictor_dropout_rate=0.1,
                 postnet_dropout_rate=0.5, init_type="xavier_uniform", init_enc_alpha=1.0,
                 init_dec_alpha=1.0, use_masking=False, use_weighted_masking=False, device=None):
        if encoder_type != "transformer":
            raise ValueError(f"{encoder_type} is not supported.")   # fastspeech2.py:187
        if decoder_type != "transformer":
            raise ValueError(f"{decoder_type} is not supported.")   # fastspeech2.py:268
        if positionwise_layer_type not in ("conv1d", "linear", "conv1d-linear"):
            raise NotImplementedError("Support only linear or conv1d.")   # encoder.py:169
        self.idim, self.odim = idim, odim
        self._adim = adim
        self.eos = idim - 1
        self.reduction_factor = reduction_factor
        self.padding_idx = 0
        self.training = True
        self._ctx = Context.get(device)
        cfg = _capi.Fs2Cfg()
        cfg.idim, cfg.odim, cfg.adim, cfg.aheads = idim, odim, adim, aheads
        cfg.elayers, cfg.eunits, cfg.dlayers, cfg.dunits = elayers, eunits, dlayers, dunits
        cfg.positionwise_conv_kernel_size = positionwise_conv_kernel_size
        cfg.positionwise_layer_type = {"conv1d": 0, "linear": 1, "conv1d-linear": 2}[positionwise_layer_type]
        cfg.duration_predictor_layers = duration_predictor_layers
        cfg.duration_predictor_chans = duration_predictor_chans
        cfg.duration_predictor_kernel_size = duration_predictor_kernel_size
        cfg.pitch_predictor_layers = pitch_predictor_layers
        cfg.pitch_predictor_chans = pitch_predictor_chans
        cfg.pitch_predictor_kernel_size = pitch_predictor_kernel_size
        cfg.energy_predictor_layers = energy_predictor_layers
        cfg.energy_predictor_chans = energy_predictor_chans
        cfg.energy_predictor_kernel_size = energy_predictor_kernel_size
        cfg.pitch_embed_kernel_size = pitch_embed_kernel_size
        cfg.energy_embed_kernel_size = energy_embed_kernel_size
        cfg.postnet_layers, cfg.postnet_chans, cfg.postnet_filts = postnet_layers, postnet_chans, postnet_filts
        cfg.use_batch_norm = 1 if use_batch_norm else 0
        cfg.use_scaled_pos_enc = 1 if use_scaled_pos_enc else 0
        cfg.encoder_normalize_before = 1 if encoder_normalize_before else 0
        cfg.decoder_normalize_before = 1 if decoder_normalize_before else 0
        cfg.encoder_concat_after = 1 if encoder_concat_after else 0
        cfg.decoder_concat_after = 1 if decoder_concat_after else 0
        cfg.reduction_factor = reduction_factor
        if spk_embed_dim is not None and spk_embed_integration_type not in ("add", "concat"):
            raise NotImplementedError("support only add or concat.")   # fastspeech2.py:584
        cfg.num_speakers = 0 if (num_speakers is None or spk_embed_dim is None) else int(num_speakers)
        cfg.spk_embed_dim = 0 if spk_embed_dim is None else int(spk_embed_dim)
        cfg.spk_embed_integration_type = 1 if spk_embed_integration_type == "concat" else 0
        if tone_embed_dim is not None and tone_embed_integration_type != "add":
            raise NotImplementedError("tone_embed_integration_type='concat': the reference's branch cannot "
                                      "broadcast the 1-D tone ids of inference (fastspeech2.py:606-610)")
        cfg.num_tones = 0 if (num_tones is None or tone_embed_dim is None) else int(num_tones)
        cfg.tone_embed_dim = 0 if tone_embed_dim is None else int(tone_embed_dim)
        cfg.tone_embed_integration_type = 0
        self.tone_embed_dim = tone_embed_dim
        self.spk_embed_dim = spk_embed_dim
        self._postnet_layers = postnet_layers
        h = C.c_void_p()
        _capi.check(self._ctx.lib.pk_fs2_create(self._ctx.handle, C.byref(cfg), C.byref(h)))
        self._h = h
        self._finalized = False
        self._last_tok, self._last_frames = [], []

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._ctx.lib.pk_fs2_destroy(h)
            except Exception:
                pass

    def set_state_dict(self, state_dict):
        set_params(self._ctx.lib.pk_fs2_set_param, self._h, state_dict)
        self._finalized = False

    def eval(self):
        self.training = False
        return self

    def set_normalizer(self, normalizer):
        """Register ZScore statistics on the engine handle.  Registering changes nothing by itself: they are
        applied only by calls that ask for it (``denormalize=True``, what ``FastSpeech2Inference`` passes), so
        ``inference()`` itself stays in the normalised domain like the reference's (fastspeech2.py:468-558)."""
        self._norm_owner = None
        if normalizer is None:
            _capi.check(self._ctx.lib.pk_fs2_set_normalizer(self._h, None, None, 0))
        else:
            mu, sigma = to_numpy_f32(normalizer.mu).reshape(-1), to_numpy_f32(normalizer.sigma).reshape(-1)
            _capi.check(self._ctx.lib.pk_fs2_set_normalizer(self._h, _capi.fptr(mu), _capi.fptr(sigma), mu.size))
        self._finalized = False

    def _finalize(self):
        if not self._finalized:
            _capi.check(self._ctx.lib.pk_fs2_finalize(self._h))
            self._finalized = True

    def set_math(self, mode):
        """'f16x3' (default: 3-term split-fp16 MFMA GEMMs, fp32-equivalent error) or 'f32' (exact fp32 MFMA)."""
        _capi.check(self._ctx.lib.pk_fs2_set_math(self._h, {"f32": 0, "f16x3": 1}[mode]))

    def set_option(self, key, value):
        """Named integer options of the engine handle (include/pk_synth.h, pk_fs2_set_option): 'ffn_planes',
        'ffn_planes_min_blocks', 'ffnp_variant', 'attn_waves'.  The library reads no environment variable."""
        _capi.check(self._ctx.lib.pk_fs2_set_option(self._h, key.encode(), int(value)))

    def set_debug(self, on=True):
        _capi.check(self._ctx.lib.pk_fs2_set_debug(self._h, 1 if on else 0))

    # -- synthesis -----------------------------------------------------------
    def encode_batch(self, texts, alpha=1.0, spk_ids=None, spembs=None, tone_ids=None, durations=None, pitch=None,
                     energy=None):
        """Phase 1: returns the per-utterance frame counts (host ints).  ``spk_ids`` (B,) ints or
        ``spembs`` (B, spk_embed_dim): speaker conditioning of a multi-speaker model (:396-402).
        ``durations`` / ``pitch`` / ``energy``: lists of per-utterance (T,) or (T, 1) arrays that stand in for the
        predictor's values (``pk_fs2_set_targets``); given durations are used as they are, ``alpha`` does not scale them."""
        ctx = Context.get(self._ctx.device)
        self._finalize()
        ids = [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t).astype(np.int64).reshape(-1)
               for t in texts]
        if durations is not None or pitch is not None or energy is not None:
            def pack(name, vals, dtype):
                if vals is None:
                    return None
                vals = [_host(v).reshape(-1) for v in vals]
                if [len(v) for v in vals] != [len(i) for i in ids]:
                    raise ValueError(f"{name}: one value per token of every utterance is needed, got lengths "
                                     f"{[len(v) for v in vals]} for {[len(i) for i in ids]} tokens")
                return np.ascontiguousarray(np.concatenate(vals).astype(dtype))
            d, p, e = pack("durations", durations, np.int64), pack("pitch", pitch, np.float32), pack(
                "energy", energy, np.float32)
            targets = (d, p, e)
        else:
            targets = None
        if self.tone_embed_dim is not None and tone_ids is not None:
            tn = [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t).astype(np.int64).reshape(-1)
                  for t in tone_ids]
            assert [len(t) for t in tn] == [len(i) for i in ids], "one tone id per token"
            tflat = np.ascontiguousarray(np.concatenate(tn))
            _capi.check(ctx.lib.pk_fs2_set_tones(self._h, tflat.ctypes.data_as(C.POINTER(C.c_int64)), tflat.size))
        if self.spk_embed_dim is not None and (spk_ids is not None or spembs is not None):
            if spembs is not None:
                e = np.ascontiguousarray(to_numpy_f32(spembs).reshape(len(ids), self.spk_embed_dim))
                _capi.check(ctx.lib.pk_fs2_set_speakers(self._h, None, _capi.fptr(e), len(ids)))
            else:
                sp = np.ascontiguousarray(np.asarray(
                    spk_ids.cpu() if isinstance(spk_ids, torch.Tensor) else spk_ids).astype(np.int64).reshape(-1))
                assert sp.size == len(ids), "one speaker id per utterance"
                _capi.check(ctx.lib.pk_fs2_set_speakers(self._h, sp.ctypes.data_as(C.POINTER(C.c_int64)), None,
                                                        len(ids)))
        lens = np.array([len(i) for i in ids], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(ids))
        frames = np.zeros(len(ids), dtype=np.int32)
        if targets is not None:      # last, so that nothing can fail between this and the encode that consumes it
            d, p, e = targets
            _capi.check(ctx.lib.pk_fs2_set_targets(
                self._h, None if d is None else d.ctypes.data_as(C.POINTER(C.c_int64)),
                None if p is None else _capi.fptr(p), None if e is None else _capi.fptr(e), flat.size))
        _capi.check(ctx.lib.pk_fs2_encode(self._h, flat.ctypes.data_as(C.POINTER(C.c_int64)),
                                          lens.ctypes.data_as(C.POINTER(C.c_int32)), len(ids),
                                          C.c_float(alpha), frames.ctypes.data_as(C.POINTER(C.c_int32))))
        self._last_tok, self._last_frames = [int(v) for v in lens], [int(v) for v in frames]
        return frames

    def decode_packed(self, denormalize=False):
        """Phase 2: packed (sum(frames), odim) device tensor of the last encode.  ``denormalize``: apply the
        registered ZScore.inverse in the output epilogue (FastSpeech2Inference.forward :668-671)."""
        ctx = Context.get(self._ctx.device)
        total = int(sum(self._last_frames))
        mel = ctx.empty((total, self.odim))
        if total:
            _capi.check(ctx.lib.pk_fs2_decode(self._h, dptr(mel), _capi.PK_APPLY_NORMALIZER if denormalize else 0))
        return mel

    def before_packed(self):
        """Packed (sum(frames), odim) ``before_outs`` (:457) of the last decode, never de-normalised."""
        ctx = Context.get(self._ctx.device)
        total = int(sum(self._last_frames))
        if self._postnet_layers == 0:        # after_outs IS before_outs (:460-461)
            return self.decode_packed(False)
        out = ctx.empty((total, self.odim))
        if total:
            _capi.check(ctx.lib.pk_fs2_read_before(self._h, dptr(out), 0))
        return out

    def read_predictions(self):
        """``(d_outs, p_outs, e_outs)`` of the last encode, one float32 (T,) host array per utterance each.  ``d_outs``: the
        integer durations of the inference branch (``alpha`` applied), or, when durations were given, the duration
        predictor's log-domain output (``DurationPredictor.forward``)."""
        n = int(sum(self._last_tok))
        d, p, e = (np.empty(n, dtype=np.float32) for _ in range(3))
        _capi.check(self._ctx.lib.pk_fs2_read_predictions(self._h, _capi.fptr(d), _capi.fptr(p), _capi.fptr(e), n))
        cuts = np.cumsum(self._last_tok)[:-1]
        return np.split(d, cuts), np.split(p, cuts), np.split(e, cuts)

    def _split(self, packed, frames):
        outs, o = [], 0
        for f in frames:
            outs.append(wrap(packed[o:o + int(f)]))
            o += int(f)
        return outs

    def inference_batch(self, texts, alpha=1.0, spk_ids=None, spembs=None, tone_ids=None, denormalize=False, *,
                        durations=None, pitch=None, energy=None):
        """One encode and one decode for a ragged batch; every utterance is evaluated as if it were alone.
        ``durations`` / ``pitch`` / ``energy`` (keyword only; each a list of per-utterance arrays or None) override the
        predicted values: read them with ``predict_batch``, edit, and synthesise with the edited ones."""
        frames = self.encode_batch(texts, alpha, spk_ids, spembs, tone_ids, durations, pitch, energy)
        return self._split(self.decode_packed(denormalize), frames)

    def predict_batch(self, texts, alpha=1.0, spk_ids=None, spembs=None, tone_ids=None):
        """Per utterance ``(durations int64 (T,), pitch (T,), energy (T,))`` of the inference branch (:423-425; the durations
        carry ``alpha``).  One encode, no decode."""
        self.encode_batch(texts, alpha, spk_ids, spembs, tone_ids)
        d, p, e = self.read_predictions()
        return [(db.astype(np.int64), pb, eb) for db, pb, eb in zip(d, p, e)]

    def teacher_forced_batch(self, texts, durations, pitch, energy, spk_ids=None, spembs=None, tone_ids=None,
                             denormalize=False, return_before=False):
        """``_forward(xs, ilens, olens, ds, ps, es, is_inference=False)`` (:433-442) for a ragged batch in one encode and one
        decode: the ground-truth-aligned mel of every utterance, (r * sum(d), odim) each (``(before_outs, after_outs)`` pairs
        with ``return_before``).  Every utterance is evaluated as if it were alone, like ``inference_batch``.  Tone ids are the
        per-token ids ``inference`` forwards."""
        if durations is None or pitch is None or energy is None:
            raise ValueError("teacher forcing needs durations, pitch and energy")
        frames = self.encode_batch(texts, 1.0, spk_ids, spembs, tone_ids, durations, pitch, energy)
        after = self._split(self.decode_packed(denormalize), frames)
        if not return_before:
            return after
        return list(zip(self._split(self.before_packed(), frames), after))

    def forward(self, text, text_lengths, speech, speech_lengths, durations, pitch, energy, tone_id=None, spembs=None,
                spk_id=None):
        """fastspeech2.py:286-375: padded batch in, ``(before_outs, after_outs, d_outs, p_outs, e_outs, ys, olens)`` out
        (padded, zeros in padded rows; ``ys`` / ``olens`` trimmed to a multiple of ``reduction_factor`` as at :369-373).

        The engine evaluates every utterance as if it were alone; the reference's batched ``forward`` lets padded rows
        reach the last valid rows of a shorter utterance through the k = 3 convolutions.  The result therefore equals the
        reference's for each utterance taken alone, and for a batch of equal lengths -- the contract ``inference_batch``
        has.  ``d_outs`` is the duration predictor's log-domain output (``DurationPredictor.forward``)."""
        if tone_id is not None:
            raise NotImplementedError(
                "tone_id in forward(): the reference's batched branch normalises the (B, T, D) tone embeddings over the "
                "TIME axis (F.normalize's default axis 1, fastspeech2.py:596), not over the features as inference()'s 1-D "
                "ids do; use teacher_forced_batch(tone_ids=...) for the per-token reading")
        r = self.reduction_factor
        xs = _host(text).astype(np.int64)
        ilens = [int(v) for v in _host(text_lengths).reshape(-1)]
        olens = np.array([int(v) for v in _host(speech_lengths).reshape(-1)], dtype=np.int64)
        ds = _host(durations).astype(np.int64)
        ps = _host(pitch).astype(np.float32).reshape(ds.shape)
        es = _host(energy).astype(np.float32).reshape(ds.shape)
        B = len(ilens)
        for b in range(B):
            if int(olens[b]) // r != int(ds[b, :ilens[b]].sum()):
                raise ValueError(f"utterance {b}: speech_lengths // reduction_factor = {int(olens[b]) // r} frames, the "
                                 f"durations sum to {int(ds[b, :ilens[b]].sum())}")
        sel = [slice(0, n) for n in ilens]
        frames = self.encode_batch(
            [xs[b, sel[b]] for b in range(B)], 1.0,
            None if spk_id is None or spembs is not None else _host(spk_id).reshape(-1),
            None if spembs is None else to_numpy_f32(spembs).reshape(B, -1), None,
            [ds[b, sel[b]] for b in range(B)], [ps[b, sel[b]] for b in range(B)], [es[b, sel[b]] for b in range(B)])
        after = self._split(self.decode_packed(False), frames)
        before = self._split(self.before_packed(), frames)
        d, p, e = self.read_predictions()
        ctx = Context.get(self._ctx.device)
        Lmax, Tmax = int(max(frames)), xs.shape[1]
        before_outs = torch.zeros((B, Lmax, self.odim), dtype=torch.float32, device=ctx.device)
        after_outs = torch.zeros_like(before_outs)
        d_outs = torch.zeros((B, Tmax), dtype=torch.float32)
        p_outs, e_outs = torch.zeros((B, Tmax, 1), dtype=torch.float32), torch.zeros((B, Tmax, 1), dtype=torch.float32)
        for b in range(B):
            before_outs[b, :int(frames[b])] = before[b]
            after_outs[b, :int(frames[b])] = after[b]
            d_outs[b, :ilens[b]] = torch.from_numpy(d[b])
            p_outs[b, :ilens[b], 0] = torch.from_numpy(p[b])
            e_outs[b, :ilens[b], 0] = torch.from_numpy(e[b])
        ys = speech
        olens_out = torch.from_numpy(olens)
        if r > 1:                                     # :369-373
            olens_out = torch.from_numpy(olens - olens % r)
            ys = ys[:, :int(olens_out.max())]
        return wrap(before_outs), wrap(after_outs), wrap(d_outs), wrap(p_outs), wrap(e_outs), ys, olens_out

    def evaluate_batch(self, text, text_lengths, speech, speech_lengths, durations, pitch, energy, spk_id=None, spembs=None,
                       use_masking=False, use_weighted_masking=False):
        """``FastSpeech2Evaluator.evaluate_core`` (fastspeech2_updater.py:123-163) on one padded batch: ``forward``, then
        ``FastSpeech2Loss`` -> ``{"l1_loss", "duration_loss", "pitch_loss", "energy_loss", "loss"}`` as Python floats (the
        means and their sum formed in float64).  The flags default to the evaluator's."""
        crit = FastSpeech2Loss(use_masking=use_masking, use_weighted_masking=use_weighted_masking)
        before_outs, after_outs, d_outs, p_outs, e_outs, ys, olens = self.forward(
            text, text_lengths, speech, speech_lengths, durations, pitch, energy, spembs=spembs, spk_id=spk_id)
        return _loss_dict(*crit.terms(after_outs, before_outs, d_outs, p_outs, e_outs, ys, durations, pitch, energy,
                                      text_lengths, olens))

    def evaluate_per_utterance(self, texts, durations, pitch, energy, target_mels, spk_ids=None, spembs=None, tone_ids=None):
        """The evaluator's five numbers of every utterance scored as a batch of one (no padding: the three masking modes
        coincide) -> list of dicts.  One ragged encode, decode and loss pass; an utterance's numbers are the same bits in any
        batch.  ``target_mels[b]`` is (r * sum(durations[b]), odim)."""
        from .losses import pair_loss_sums
        ctx = Context.get(self._ctx.device)
        frames = self.encode_batch(texts, 1.0, spk_ids, spembs, tone_ids, durations, pitch, energy)
        tgts = [ctx.to_device(t) for t in target_mels]
        if len(tgts) != len(frames):
            raise ValueError(f"{len(frames)} utterances, {len(tgts)} target mels")
        for b, t in enumerate(tgts):
            if t.dim() != 2 or tuple(t.shape) != (int(frames[b]), self.odim) or frames[b] == 0:
                raise ValueError(f"pair {b}: target mel {tuple(t.shape)}, the durations give {int(frames[b])} frames of "
                                 f"{self.odim} bins (none cannot be averaged)")
        after, before = self.decode_packed(False), self.before_packed()
        ys = torch.cat(tgts)
        l1 = pair_loss_sums(before, ys, frames)[:, 0] + pair_loss_sums(after, ys, frames)[:, 0]
        d, p, e = (np.concatenate(v) for v in self.read_predictions())
        tok = np.asarray(self._last_tok, np.int64)
        cat = lambda vals, dt: np.concatenate([_host(v).reshape(-1) for v in vals]).astype(dt)   # noqa: E731
        log_ds = DurationPredictorLoss().log_targets(cat(durations, np.int64))
        dur = pair_loss_sums(d, log_ds, tok, width=1)[:, 1]
        pit = pair_loss_sums(p, cat(pitch, np.float32), tok, width=1)[:, 1]
        ene = pair_loss_sums(e, cat(energy, np.float32), tok, width=1)[:, 1]
        n = frames.astype(np.float64) * self.odim
        return [_loss_dict(l1[b] / n[b], dur[b] / tok[b], pit[b] / tok[b], ene[b] / tok[b]) for b in range(len(frames))]

    def inference(self, text, speech=None, durations=None, pitch=None, energy=None, alpha=1.0,
                  use_teacher_forcing=False, spembs=None, spk_id=None, tone_id=None, denormalize=False):
        """(T,) int64 -> (L, odim); fastspeech2.py:468-558.  ``use_teacher_forcing=True`` needs ``durations`` (T,), ``pitch``
        and ``energy`` ((T,) or (T, 1)) and computes ``_forward(ds, ps, es, is_inference=False)`` with them for any T
        (``alpha`` is not applied, as in the reference; its ``if durations:`` at :516 is what stops the reference's own
        wrapper for T > 1).  Without the switch the three are ignored, as in the reference."""
        kw = {}
        if use_teacher_forcing:
            if durations is None or pitch is None or energy is None:
                raise ValueError("use_teacher_forcing=True needs durations, pitch and energy")
            kw = dict(durations=[durations], pitch=[pitch], energy=[energy])
        tones = None if tone_id is None else [tone_id]   # (T,) ids, forwarded un-batched by the reference (:546,556)
        if spembs is not None:      # (spk_embed_dim,), unsqueezed by the reference (:541-542)
            return self.inference_batch([text], alpha, spembs=to_numpy_f32(spembs).reshape(1, -1), tone_ids=tones,
                                        denormalize=denormalize, **kw)[0]
        if spk_id is not None:
            sid = np.asarray(spk_id.cpu() if isinstance(spk_id, torch.Tensor) else spk_id).reshape(-1)[:1]
            return self.inference_batch([text], alpha, spk_ids=sid, tone_ids=tones, denormalize=denormalize, **kw)[0]
        return self.inference_batch([text], alpha, tone_ids=tones, denormalize=denormalize, **kw)[0]

    def debug_tap(self, what, b):
        n_rows = self._last_tok[b] if what <= 3 else self._last_frames[b]
        width = {0: -1, 1: 1, 2: 1, 3: 1, 4: -1, 5: -1, 6: self.odim}[what]
        if width == -1:
            width = self._adim
        out = np.empty((n_rows, width), dtype=np.float32)
        _capi.check(self._ctx.lib.pk_fs2_debug_read(self._h, what, b, _capi.fptr(out), out.size))
        return out[:, 0] if width == 1 else out


class DurationPredictorLoss:
    """duration_predictor.py:140-184: MSE between the predictor's log-domain outputs and ``log(targets + offset)``.  The
    targets' logarithm is taken in float32 as the reference takes it; the squared differences are summed by
    ``pk_pair_loss_run`` and divided on the host.  ``reduction`` "mean" or "sum" give a 0-d float32 device tensor, "none" the
    elementwise tensor (plain tensor arithmetic: nothing is reduced)."""

    def __init__(self, offset=1.0, reduction="mean"):
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"reduction {reduction!r}")
        self.offset, self.reduction = offset, reduction

    def log_targets(self, targets):
        ctx = Context.get()
        return torch.log(ctx.to_device(targets, dtype=torch.float32) + self.offset)

    def forward(self, outputs, targets):
        from .losses import pair_loss_sums, scalar
        ctx = Context.get()
        o, t = ctx.to_device(outputs), self.log_targets(targets)
        if o.shape != t.shape:
            raise ValueError(f"outputs {tuple(o.shape)} against targets {tuple(t.shape)}")
        if self.reduction == "none":
            return wrap((o - t) ** 2)
        s = pair_loss_sums(o.reshape(-1), t.reshape(-1), [o.numel()], width=1)[0, 1]
        return scalar(s / o.numel() if self.reduction == "mean" else s, ctx)

    __call__ = forward


class FastSpeech2Loss:
    """fastspeech2.py:674-812 with the reference's eleven arguments -> ``(l1_loss, duration_loss, pitch_loss,
    energy_loss)``, 0-d float32 device tensors.  ``use_masking``: means over the valid frames / tokens; neither flag: means
    over the padded rectangles as given; ``use_weighted_masking``: every utterance's sum divided by L_b * B * odim (mel) or
    T_b * B (token terms).  ``after_outs=None`` leaves the L1 term to ``before_outs`` (:759, :777).  The device leaves
    float64 sums per utterance (``pk_pair_loss_run``, the predictors' terms at W = 1); the means are formed on the host."""

    def __init__(self, use_masking=True, use_weighted_masking=False):
        from .losses import masking_mode
        self._mode = masking_mode(use_masking, use_weighted_masking)
        self.use_masking, self.use_weighted_masking = use_masking, use_weighted_masking
        self.duration_criterion = DurationPredictorLoss(reduction="none" if use_weighted_masking else "mean")

    def terms(self, after_outs, before_outs, d_outs, p_outs, e_outs, ys, ds, ps, es, ilens, olens):
        """The four numbers in float64."""
        from .losses import masked_pair_means
        ctx = Context.get()
        flat = lambda x: ctx.to_device(x).reshape(x.shape[0], -1)   # noqa: E731  (B, Tmax, 1) -> (B, Tmax)
        l1 = masked_pair_means(before_outs, ys, olens, self._mode)[0]
        if after_outs is not None:
            l1 += masked_pair_means(after_outs, ys, olens, self._mode)[0]
        dur = masked_pair_means(flat(d_outs), self.duration_criterion.log_targets(flat(ds)), ilens, self._mode)[1]
        pitch = masked_pair_means(flat(p_outs), flat(ps), ilens, self._mode)[1]
        energy = masked_pair_means(flat(e_outs), flat(es), ilens, self._mode)[1]
        return l1, dur, pitch, energy

    def forward(self, after_outs, before_outs, d_outs, p_outs, e_outs, ys, ds, ps, es, ilens, olens):
        from .losses import scalar
        return tuple(scalar(v) for v in self.terms(after_outs, before_outs, d_outs, p_outs, e_outs, ys, ds, ps, es, ilens,
                                                   olens))

    __call__ = forward


def _loss_dict(l1, dur, pitch, energy):
    return {"l1_loss": float(l1), "duration_loss": float(dur), "pitch_loss": float(pitch), "energy_loss": float(energy),
            "loss": float(l1 + dur + pitch + energy)}


class FastSpeech2Inference:
    """FastSpeech2Inference (fastspeech2.py:662-671): inference then normalizer.inverse."""

    def __init__(self, normalizer, model):
        self.normalizer = normalizer
        self.acoustic_model = model
        self.bind()

    def bind(self):
        """Make this wrapper's statistics the ones registered on the model's engine handle (a no-op unless
        another wrapper around the same model registered different ones since).  The model's own
        ``inference()`` is unaffected either way."""
        m = self.acoustic_model
        if getattr(m, "_norm_owner", None) is not self:
            m.set_normalizer(self.normalizer)
            m._norm_owner = self
        return m

    def forward(self, text, spk_id=None, alpha=1.0):
        return self.bind().inference(text, spk_id=spk_id, alpha=alpha, denormalize=True)

    __call__ = forward

    def eval(self):
        return self
