"""TransformerTTS acoustic model behind the reference's Python API.

Mirrors parakeet/models/transformer_tts/transformer_tts.py: ``TransformerTTS`` (constructor kwargs :172-250,
``set_state_dict``, ``eval``, ``inference`` :511-647 -> (outs, probs, att_ws)) and ``TransformerTTSInference``
(:757-767).  All arithmetic runs in libpk_synth.so (csrc/tts.hip on the shared transformer machinery of csrc/fft.hip).
``inference(..., use_teacher_forcing=True)`` runs the decoder as one parallel pass over the teacher spectrogram
(csrc/tts_teacher.hip); ``forward`` (:381-460) is that pass on a padded batch, with the stop logits and the outputs before
the postnet.  ``TransformerTTSLoss`` (:770-871), ``GuidedAttentionLoss`` (:874-1035) and ``GuidedMultiHeadAttentionLoss``
(:1038-1082) reduce on the engine (csrc/seq_loss.hip); ``evaluate_batch`` is ``TransformerTTSEvaluator.evaluate_core``.
Gradients and updaters are out of scope.

The reference's decoder prenet keeps dropout on at inference (modules/tacotron2/decoder.py:78-81), so its output
depends on Paddle's random generator.  Here the mask comes from the engine's counter-based dropout stream
(include/pk_synth.h): ``seed=`` selects it, the same seed gives the same spectrogram on any batch composition.

Extensions (supersets): ``inference_batch`` decodes a ragged batch in lockstep; ``teacher_forced_batch`` teacher-forces
a ragged batch in one pass; ``seed`` / ``dropout``.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, set_params, to_numpy_f32, wrap


def _ids(v):
    if hasattr(v, "numpy") and not isinstance(v, (np.ndarray, torch.Tensor)):
        v = v.numpy()
    return np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v).astype(np.int64).reshape(-1)


class TransformerTTS:
    def __init__(self, idim, odim, embed_dim=512, eprenet_conv_layers=3, eprenet_conv_chans=256, eprenet_conv_filts=5,
                 dprenet_layers=2, dprenet_units=256, elayers=6, eunits=1024, adim=512, aheads=4, dlayers=6,
                 dunits=1024, postnet_layers=5, postnet_chans=256, postnet_filts=5, positionwise_layer_type="conv1d",
                 positionwise_conv_kernel_size=1, use_scaled_pos_enc=True, use_batch_norm=True,
                 encoder_normalize_before=True, decoder_normalize_before=True, encoder_concat_after=False,
                 decoder_concat_after=False, reduction_factor=1, spk_embed_dim=None, spk_embed_integration_type="add",
                 use_gst=False, gst_tokens=10, gst_heads=4, gst_conv_layers=6,
                 gst_conv_chans_list=(32, 32, 64, 64, 128, 128), gst_conv_kernel_size=3, gst_conv_stride=2,
                 gst_gru_layers=1, gst_gru_units=128, transformer_enc_dropout_rate=0.1,
                 transformer_enc_positional_dropout_rate=0.1, transformer_enc_attn_dropout_rate=0.1,
                 transformer_dec_dropout_rate=0.1, transformer_dec_positional_dropout_rate=0.1,
                 transformer_dec_attn_dropout_rate=0.1, transformer_enc_dec_attn_dropout_rate=0.1,
                 eprenet_dropout_rate=0.5, dprenet_dropout_rate=0.5, postnet_dropout_rate=0.5,
                 init_type="xavier_uniform", init_enc_alpha=1.0, init_dec_alpha=1.0, use_guided_attn_loss=True,
                 num_heads_applied_guided_attn=2, num_layers_applied_guided_attn=2, device=None):
        if positionwise_layer_type not in ("conv1d", "linear", "conv1d-linear"):
            raise NotImplementedError("Support only linear or conv1d.")   # encoder.py:169
        self.idim, self.odim = idim, odim
        self.eos = idim - 1
        self.reduction_factor = reduction_factor
        self.padding_idx = 0
        self.training = True
        self._adim, self._aheads, self._dlayers = adim, aheads, dlayers
        self.use_scaled_pos_enc = bool(use_scaled_pos_enc)
        self.use_guided_attn_loss = use_guided_attn_loss
        self.num_layers_applied_guided_attn = elayers if num_layers_applied_guided_attn == -1 else num_layers_applied_guided_attn
        self.num_heads_applied_guided_attn = aheads if num_heads_applied_guided_attn == -1 else num_heads_applied_guided_attn
        self._alphas = {}
        self.spk_embed_dim = spk_embed_dim
        if spk_embed_dim is not None and spk_embed_integration_type not in ("add", "concat"):
            raise NotImplementedError("support only add or concat.")   # transformer_tts.py:753
        self._ctx = Context.get(device)
        cfg = _capi.TtsCfg()
        cfg.idim, cfg.odim = idim, odim
        cfg.embed_dim, cfg.eprenet_conv_layers = embed_dim, eprenet_conv_layers
        cfg.eprenet_conv_chans, cfg.eprenet_conv_filts = eprenet_conv_chans, eprenet_conv_filts
        cfg.dprenet_layers, cfg.dprenet_units = dprenet_layers, dprenet_units
        cfg.adim, cfg.aheads = adim, aheads
        cfg.elayers, cfg.eunits, cfg.dlayers, cfg.dunits = elayers, eunits, dlayers, dunits
        cfg.postnet_layers, cfg.postnet_chans, cfg.postnet_filts = postnet_layers, postnet_chans, postnet_filts
        cfg.positionwise_layer_type = {"conv1d": 0, "linear": 1, "conv1d-linear": 2}[positionwise_layer_type]
        cfg.positionwise_conv_kernel_size = positionwise_conv_kernel_size
        cfg.use_scaled_pos_enc = 1 if use_scaled_pos_enc else 0
        cfg.use_batch_norm = 1 if use_batch_norm else 0
        cfg.encoder_normalize_before = 1 if encoder_normalize_before else 0
        cfg.decoder_normalize_before = 1 if decoder_normalize_before else 0
        cfg.encoder_concat_after = 1 if encoder_concat_after else 0
        cfg.decoder_concat_after = 1 if decoder_concat_after else 0
        cfg.reduction_factor = reduction_factor
        cfg.spk_embed_dim = 0 if spk_embed_dim is None else int(spk_embed_dim)
        cfg.use_gst = 1 if use_gst else 0
        self.use_gst = bool(use_gst)
        if use_gst:
            chans = [int(v) for v in gst_conv_chans_list]
            if len(chans) != gst_conv_layers:   # style_encoder.py:153-155
                raise ValueError("the number of conv layers and length of channels list must be the same.")
            if len(chans) > 8:
                raise NotImplementedError("at most 8 reference-encoder conv layers")
            cfg.gst_tokens, cfg.gst_heads = gst_tokens, gst_heads
            cfg.gst_conv_layers, cfg.gst_conv_kernel_size, cfg.gst_conv_stride = gst_conv_layers, gst_conv_kernel_size, gst_conv_stride
            cfg.gst_gru_layers, cfg.gst_gru_units = gst_gru_layers, gst_gru_units
            for i, v in enumerate(chans):
                cfg.gst_conv_chans[i] = v
        cfg.spk_embed_integration_type = 1 if spk_embed_integration_type == "concat" else 0
        h = C.c_void_p()
        _capi.check(self._ctx.lib.pk_tts_create(self._ctx.handle, C.byref(cfg), C.byref(h)))
        self._h = h
        self._finalized = False
        self._last_tok, self._last_frames = [], []

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._ctx.lib.pk_tts_destroy(h)
            except Exception:
                pass

    def set_state_dict(self, state_dict):
        set_params(self._ctx.lib.pk_tts_set_param, self._h, state_dict)
        for name, v in state_dict.items():      # ScaledPositionalEncoding.alpha of encoder.embed[-1] / decoder.embed[-1]
            if name.endswith(".alpha") and name.split(".")[0] in ("encoder", "decoder"):
                self._alphas[name.split(".")[0]] = float(to_numpy_f32(v).reshape(-1)[0])
        self._finalized = False

    def eval(self):
        self.training = False
        return self

    def set_normalizer(self, normalizer):
        """Register ZScore statistics; applied only by calls passing ``denormalize=True`` (TransformerTTSInference)."""
        self._norm_owner = None
        if normalizer is None:
            _capi.check(self._ctx.lib.pk_tts_set_normalizer(self._h, None, None, 0))
        else:
            mu, sigma = to_numpy_f32(normalizer.mu).reshape(-1), to_numpy_f32(normalizer.sigma).reshape(-1)
            _capi.check(self._ctx.lib.pk_tts_set_normalizer(self._h, _capi.fptr(mu), _capi.fptr(sigma), mu.size))
        self._finalized = False

    def set_math(self, mode):
        """'f16x3' (default: split-fp16 MFMA GEMMs, fp32-equivalent error) or 'f32' (exact fp32 MFMA)."""
        _capi.check(self._ctx.lib.pk_tts_set_math(self._h, {"f32": 0, "f16x3": 1}[mode]))

    def set_option(self, key, value):
        """Named integer options of the engine handle (include/pk_synth.h, pk_tts_set_option): 'kv_prefix' and the FFT-stack
        options of FastSpeech2.set_option."""
        _capi.check(self._ctx.lib.pk_tts_set_option(self._h, key.encode(), int(value)))

    def set_dropout(self, on):
        """False switches the decoder prenet's dropout off (deterministic; not what the reference computes)."""
        _capi.check(self._ctx.lib.pk_tts_set_dropout(self._h, 1 if on else 0))

    def _finalize(self):
        if not self._finalized:
            _capi.check(self._ctx.lib.pk_tts_finalize(self._h))
            self._finalized = True

    def inference_batch(self, texts, threshold=0.5, minlenratio=0.0, maxlenratio=10.0, seeds=None,
                        return_att=True, denormalize=False, spembs=None, speech=None):
        """Lists of (T_b,) token ids (without <eos>) -> list of (outs (L_b, odim), probs (L_b,),
        att_ws (dlayers, aheads, L_b / reduction_factor, T_b + 1) or None) device tensors.  ``spembs``: (B, spk_embed_dim), one speaker
        embedding per utterance, for a model built with ``spk_embed_dim``.  ``speech``: list of (L_b, odim) reference
        spectrograms, one per utterance, for a ``use_gst`` model."""
        ctx = Context.get(self._ctx.device)
        self._finalize()
        if speech is not None and self.use_gst:
            refs = [to_numpy_f32(y).reshape(-1, self.odim) for y in speech]
            if len(refs) != len(texts):
                raise ValueError("one reference spectrogram per utterance")
            rl = np.array([r.shape[0] for r in refs], dtype=np.int32)
            flat_ref = np.ascontiguousarray(np.concatenate(refs, axis=0))
            _capi.check(ctx.lib.pk_tts_set_style_reference(self._h, _capi.fptr(flat_ref), rl.ctypes.data_as(C.POINTER(C.c_int32)),
                                                           len(refs)))
        if spembs is not None:
            e = to_numpy_f32(spembs).reshape(len(texts), -1)
            if e.shape[1] != (self.spk_embed_dim or 0):
                raise ValueError(f"spembs has {e.shape[1]} columns, the model was built with spk_embed_dim={self.spk_embed_dim}")
            _capi.check(ctx.lib.pk_tts_set_speakers(self._h, _capi.fptr(e), e.shape[0]))
        ids = [_ids(t) for t in texts]
        B = len(ids)
        lens = np.array([len(i) for i in ids], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(ids)) if lens.sum() else np.zeros(1, np.int64)
        frames = np.zeros(B, dtype=np.int32)
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
            assert sd.size == B, "one dropout seed per utterance"
        flags = _capi.PK_TTS_KEEP_ATT if return_att else 0
        _capi.check(ctx.lib.pk_tts_infer(self._h, flat.ctypes.data_as(C.POINTER(C.c_int64)),
                                         lens.ctypes.data_as(C.POINTER(C.c_int32)), B, float(threshold),
                                         float(minlenratio), float(maxlenratio),
                                         None if sd is None else sd.ctypes.data_as(C.POINTER(C.c_uint64)), flags,
                                         frames.ctypes.data_as(C.POINTER(C.c_int32))))
        self._last_tok, self._last_frames = [int(v) + 1 for v in lens], [int(v) for v in frames]
        steps = [L // self.reduction_factor for L in self._last_frames]     # one attention row per decoder step
        total = int(frames.sum())
        mel = ctx.empty((total, self.odim))
        probs = ctx.empty((total,))
        att = None
        if return_att:
            n_att = sum(self._dlayers * self._aheads * S * T for S, T in zip(steps, self._last_tok))
            att = ctx.empty((n_att,))
        _capi.check(ctx.lib.pk_tts_read(self._h, dptr(mel), dptr(probs), None if att is None else dptr(att),
                                        _capi.PK_APPLY_NORMALIZER if denormalize else 0))
        outs, o, oa = [], 0, 0
        for L, S, T in zip(self._last_frames, steps, self._last_tok):
            a = None
            if att is not None:
                n = self._dlayers * self._aheads * S * T
                a = wrap(att[oa:oa + n].view(self._dlayers, self._aheads, S, T))
                oa += n
            outs.append((wrap(mel[o:o + L]), wrap(probs[o:o + L]), a))
            o += L
        return outs

    def teacher_forced_batch(self, texts, speech, seeds=None, spembs=None, return_att=True, denormalize=False):
        """Teacher forcing for a ragged batch (transformer_tts.py:567-579): lists of (T_b,) token ids (without <eos>) and
        (L_b, odim) teacher spectrograms in the model's normalised space -> list of (outs ((L_b // r) * r, odim),
        att_ws (dlayers, aheads, L_b // r, T_b + 1) or None) device tensors.  The style embedding of a ``use_gst`` model
        comes from the teacher spectrogram (:475-477).  ``spembs``: (B, spk_embed_dim) for a model built with
        ``spk_embed_dim``.  The stop probabilities of the teacher-forced rows are kept as ``last_probs``."""
        ctx = Context.get(self._ctx.device)
        self._finalize()
        ys = [to_numpy_f32(y) for y in speech]
        if len(ys) != len(texts):
            raise ValueError("one teacher spectrogram per utterance")
        for y in ys:
            if y.ndim != 2 or y.shape[1] != self.odim:
                raise ValueError(f"teacher spectrogram of shape {tuple(y.shape)}, expected (L, {self.odim})")
            if y.shape[0] < self.reduction_factor:
                raise ValueError(f"teacher spectrogram of {y.shape[0]} frames, fewer than reduction_factor "
                                 f"{self.reduction_factor}")
        if spembs is not None:
            e = to_numpy_f32(spembs).reshape(len(texts), -1)
            if e.shape[1] != (self.spk_embed_dim or 0):
                raise ValueError(f"spembs has {e.shape[1]} columns, the model was built with spk_embed_dim={self.spk_embed_dim}")
            _capi.check(ctx.lib.pk_tts_set_speakers(self._h, _capi.fptr(e), e.shape[0]))
        else:
            _capi.check(ctx.lib.pk_tts_set_speakers(self._h, None, 0))
        ids = [_ids(t) for t in texts]
        B = len(ids)
        lens = np.array([len(i) for i in ids], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(ids)) if lens.sum() else np.zeros(1, np.int64)
        ylens = np.array([y.shape[0] for y in ys], dtype=np.int32)
        flat_y = np.ascontiguousarray(np.concatenate(ys, axis=0))
        frames = np.zeros(B, dtype=np.int32)
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
            assert sd.size == B, "one dropout seed per utterance"
        flags = _capi.PK_HOST_IO | (_capi.PK_TTS_KEEP_ATT if return_att else 0)
        _capi.check(ctx.lib.pk_tts_teacher(self._h, flat.ctypes.data_as(C.POINTER(C.c_int64)),
                                           lens.ctypes.data_as(C.POINTER(C.c_int32)), B, _capi.fptr(flat_y),
                                           ylens.ctypes.data_as(C.POINTER(C.c_int32)),
                                           None if sd is None else sd.ctypes.data_as(C.POINTER(C.c_uint64)), flags,
                                           frames.ctypes.data_as(C.POINTER(C.c_int32))))
        self._last_tok, self._last_frames = [int(v) + 1 for v in lens], [int(v) for v in frames]
        rows = [L // self.reduction_factor for L in self._last_frames]
        total = int(frames.sum())
        mel = ctx.empty((total, self.odim))
        probs = ctx.empty((total,))
        att = None
        if return_att:
            att = ctx.empty((sum(self._dlayers * self._aheads * S * T for S, T in zip(rows, self._last_tok)),))
        _capi.check(ctx.lib.pk_tts_read(self._h, dptr(mel), dptr(probs), None if att is None else dptr(att),
                                        _capi.PK_APPLY_NORMALIZER if denormalize else 0))
        outs, o, oa = [], 0, 0
        self.last_probs = []
        for L, S, T in zip(self._last_frames, rows, self._last_tok):
            a = None
            if att is not None:
                n = self._dlayers * self._aheads * S * T
                a = wrap(att[oa:oa + n].view(self._dlayers, self._aheads, S, T))
                oa += n
            outs.append((wrap(mel[o:o + L]), a))
            self.last_probs.append(wrap(probs[o:o + L]))
            o += L
        return outs

    def durations_batch(self, texts, speech, seeds=None, spembs=None, map="focus", return_focus=False):
        """Token durations from the teacher-forced encoder-decoder attention: ``teacher_forced_batch``, one
        (layer, head) map per utterance -- ``map="focus"``: the one with the largest focus rate (``alignment.select_map``), or
        a ``(layer, head)`` pair for all --, then ``alignment.durations_from_attention`` on it with the <eos> column merged into
        the last token and the counts multiplied by ``reduction_factor``.  The maps never leave the device.  Returns
        ``(durations, score)``: a list of (T_b,) int32 numpy arrays summing to (L_b // r) * r frames, and the (B,) float64 path
        scores (with ``return_focus`` also the (B,) float64 focus rates of the maps used); the maps used are kept as
        ``last_maps``, a list of (layer, head).  Needs T_b + 1 <= L_b // r."""
        from .alignment import durations_from_attention, focus_rate, select_map
        if not (isinstance(map, str) and map == "focus"):
            try:
                layer, head = (int(v) for v in map)
            except (TypeError, ValueError):
                raise ValueError(f'map must be "focus" or a (layer, head) pair, got {map!r}') from None
            if not (0 <= layer < self._dlayers and 0 <= head < self._aheads):
                raise ValueError(f"map ({layer}, {head}) outside the model's {self._dlayers} layers x {self._aheads} heads")
        outs = self.teacher_forced_batch(texts, speech, seeds=seeds, spembs=spembs, return_att=True)
        atts = [a for _, a in outs]
        picks = select_map(atts) if isinstance(map, str) else [(layer, head)] * len(atts)
        self.last_maps = picks
        used = [a[l, h] for a, (l, h) in zip(atts, picks)]
        res = durations_from_attention(used, reduction_factor=self.reduction_factor, merge_last=True)
        return res + (np.array([float(f) for f in focus_rate(used)]),) if return_focus else res

    def _read_teacher(self):
        """Packed ``before_outs`` (sum frames, odim) and stop ``logits`` (sum frames,) of the last ``teacher_forced_batch``."""
        ctx = Context.get(self._ctx.device)
        total = int(sum(self._last_frames))
        before, logits = ctx.empty((total, self.odim)), ctx.empty((total,))
        _capi.check(ctx.lib.pk_tts_read_teacher(self._h, dptr(before), dptr(logits), 0))
        return before, logits

    def forward(self, text, text_lengths, speech, speech_lengths, spembs=None, seeds=None):
        """transformer_tts.py:381-460 on a padded batch: text (B, Tmax) ids without <eos>, text_lengths (B,), speech
        (B, Lmax, odim) in the model's normalised space, speech_lengths (B,) ->
        ``(after_outs, before_outs, logits, ys, labels, olens, ilens, need_dict)``.

        <eos> is appended (``ilens = text_lengths + 1``); ``labels`` (B, max(speech_lengths)) are 1 at each utterance's last
        frame and in the padding; with ``reduction_factor`` r > 1, ``olens`` drop to multiples of r, ``ys`` and ``labels`` are
        cut to max(olens) and ``labels[:, -1] = 1`` (:444-450).  ``after_outs`` / ``before_outs`` (B, L, odim) and ``logits``
        (B, L) are as long as ``ys`` and zero past each utterance's (speech_lengths // r) * r frames.

        Like ``FastSpeech2.forward``, every utterance is evaluated as if it were alone (the reference's padded batch lets
        padding reach valid rows through the prenet convolutions and the postnet): the result equals the reference's for
        B = 1 and for batches of equal lengths.  The decoder prenet's dropout stays on; ``seeds`` (B,) selects each
        utterance's stream.

        ``need_dict`` cannot carry the reference's Paddle modules; it is a plain dict of what the evaluator reads from them:
        ``num_heads_applied_guided_attn``, ``num_layers_applied_guided_attn``, ``use_scaled_pos_enc``, ``encoder_alpha`` and
        ``decoder_alpha`` (floats; None without scaled positional encoding), and ``enc_dec_att_ws``: the encoder-decoder
        attention weights of every decoder layer and head, (B, dlayers, aheads, L // r, Tmax + 1), zero-padded.  The
        self-attention weights of encoder and decoder are not kept by the engine."""
        r = self.reduction_factor
        xs = np.asarray(text.cpu() if isinstance(text, torch.Tensor) else text).astype(np.int64)
        sp = to_numpy_f32(speech)
        tl, ol = _ids(text_lengths), _ids(speech_lengths)
        if xs.ndim != 2 or sp.ndim != 3 or sp.shape[2] != self.odim or len({xs.shape[0], sp.shape[0], tl.size, ol.size}) != 1:
            raise ValueError(f"forward: text {xs.shape}, text_lengths {tl.shape}, speech {sp.shape}, speech_lengths {ol.shape}")
        B = xs.shape[0]
        if (tl < 0).any() or (tl > xs.shape[1]).any() or (ol < max(r, 1)).any() or (ol > sp.shape[1]).any():
            raise ValueError("forward: text_lengths / speech_lengths out of range")
        outs = self.teacher_forced_batch([xs[b, :tl[b]] for b in range(B)], [sp[b, :ol[b]] for b in range(B)], seeds,
                                         spembs, True, False)
        before, logits = self._read_teacher()
        frames = self._last_frames
        ilens = tl + 1
        # labels for stop prediction (:431-435): make_pad_mask(olens - 1), one more column of ones
        labels = (np.arange(int(ol.max()))[None, :] >= (ol[:, None] - 1)).astype(np.float32)
        ys, olens = speech, ol
        if r > 1:                                            # :444-450
            olens = ol - ol % r
            ys = ys[:, :int(olens.max())]
            labels = labels[:, :int(olens.max())].copy()
            labels[:, -1] = 1.0
        L = int(ys.shape[1])
        ctx = Context.get(self._ctx.device)
        after_outs = torch.zeros((B, L, self.odim), device=ctx.device)
        before_outs = torch.zeros_like(after_outs)
        logit_outs = torch.zeros((B, L), device=ctx.device)
        att = torch.zeros((B, self._dlayers, self._aheads, L // r, xs.shape[1] + 1), device=ctx.device)
        o = 0
        for b, (mel, a) in enumerate(outs):
            n = int(frames[b])
            after_outs[b, :n] = mel
            before_outs[b, :n] = before[o:o + n]
            logit_outs[b, :n] = logits[o:o + n]
            att[b, :, :, :a.shape[2], :a.shape[3]] = a
            o += n
        need_dict = {"num_heads_applied_guided_attn": self.num_heads_applied_guided_attn,
                     "num_layers_applied_guided_attn": self.num_layers_applied_guided_attn,
                     "use_scaled_pos_enc": self.use_scaled_pos_enc,
                     "encoder_alpha": self._alphas.get("encoder") if self.use_scaled_pos_enc else None,
                     "decoder_alpha": self._alphas.get("decoder") if self.use_scaled_pos_enc else None,
                     "enc_dec_att_ws": wrap(att)}
        return (wrap(after_outs), wrap(before_outs), wrap(logit_outs), ys, wrap(torch.from_numpy(labels).to(ctx.device)),
                torch.from_numpy(olens.copy()), torch.from_numpy(ilens), need_dict)

    __call__ = forward

    def _guided_setup(self, use_guided_attn_loss, modules_applied_guided_attn):
        if not use_guided_attn_loss:
            return False
        if isinstance(modules_applied_guided_attn, str) or not isinstance(modules_applied_guided_attn, (list, tuple)):
            raise TypeError("modules_applied_guided_attn must be a list or tuple of module names; a bare string would be "
                            "searched for substrings (the reference's default (\"encoder-decoder\") is one, and selects all "
                            "three modules that way)")
        for m in modules_applied_guided_attn:
            if m in ("encoder", "decoder"):
                raise NotImplementedError(f"guided attention over the {m}'s self-attention: the engine's fused "
                                          "self-attention never stores those probabilities")
            if m != "encoder-decoder":
                raise ValueError(f"unknown module {m!r} in modules_applied_guided_attn")
        if "encoder-decoder" not in modules_applied_guided_attn:
            return False
        if self.reduction_factor > 1:
            raise NotImplementedError("the guided attention term with reduction_factor > 1: the reference passes un-thinned "
                                      "olens against L // r attention rows and cannot run it either")
        return True

    def _selected_maps(self, att, axis):
        """The LAST num_layers_applied_guided_attn decoder layers and the FIRST num_heads_applied_guided_attn heads
        (transformer_tts_updater.py:294-305), layers and heads merged into one axis."""
        n, m = int(self.num_layers_applied_guided_attn), int(self.num_heads_applied_guided_attn)
        a = att.as_subclass(torch.Tensor)
        lay = slice(max(self._dlayers - n, 0), self._dlayers)
        a = a[:, lay, :m] if axis == 2 else a[lay, :m]
        return a.reshape(a.shape[:axis - 1] + (-1,) + a.shape[axis + 1:])

    def _alpha_entries(self):
        if not self.use_scaled_pos_enc:
            return {}
        return {"encoder_alpha": self._alphas.get("encoder"), "decoder_alpha": self._alphas.get("decoder")}

    def evaluate_batch(self, text, text_lengths, speech, speech_lengths, spembs=None, seeds=None, *, use_masking=False,
                       use_weighted_masking=False, bce_pos_weight=5.0, loss_type="L1", use_guided_attn_loss=True,
                       modules_applied_guided_attn=("encoder-decoder",), guided_attn_loss_sigma=0.4,
                       guided_attn_loss_lambda=1.0):
        """``TransformerTTSEvaluator.evaluate_core`` (transformer_tts_updater.py:222-322) on one padded batch: ``forward``,
        ``TransformerTTSLoss`` and, over the encoder-decoder attention of the last ``num_layers_applied_guided_attn``
        layers' first ``num_heads_applied_guided_attn`` heads, ``GuidedMultiHeadAttentionLoss`` -> dict of Python floats:
        ``bce_loss``, ``l1_loss``, ``l2_loss``, ``enc_dec_attn_loss`` (with the guided term), ``encoder_alpha`` /
        ``decoder_alpha`` (with scaled positional encoding) and ``loss`` (``loss_type`` "L1", "L2" or "L1+L2", plus the
        guided term).  ``modules_applied_guided_attn`` must be a list or tuple (TypeError for a bare string); "encoder" or
        "decoder" in it, and the guided term with ``reduction_factor`` > 1, raise NotImplementedError."""
        if loss_type not in ("L1", "L2", "L1+L2"):
            raise ValueError("unknown --loss-type " + str(loss_type))
        guided = self._guided_setup(use_guided_attn_loss, modules_applied_guided_attn)
        crit = TransformerTTSLoss(use_masking, use_weighted_masking, bce_pos_weight)
        after_outs, before_outs, logits, ys, labels, olens, ilens, need = self.forward(text, text_lengths, speech,
                                                                                      speech_lengths, spembs, seeds)
        l1, l2, bce = crit.terms(after_outs, before_outs, logits, ys, labels, olens)
        out = {"bce_loss": bce, "l1_loss": l1, "l2_loss": l2}
        loss = {"L1": l1, "L2": l2, "L1+L2": l1 + l2}[loss_type] + bce
        if guided:
            att_ws = self._selected_maps(need["enc_dec_att_ws"], 2)
            out["enc_dec_attn_loss"] = GuidedMultiHeadAttentionLoss(guided_attn_loss_sigma, guided_attn_loss_lambda).term(
                att_ws, ilens, olens)
            loss = loss + out["enc_dec_attn_loss"]
        out.update(self._alpha_entries())
        out["loss"] = loss
        return {k: float(v) for k, v in out.items()}

    def evaluate_per_utterance(self, texts, speech, spembs=None, seeds=None, *, bce_pos_weight=5.0, loss_type="L1",
                               use_guided_attn_loss=True, modules_applied_guided_attn=("encoder-decoder",),
                               guided_attn_loss_sigma=0.4, guided_attn_loss_lambda=1.0):
        """The evaluator's numbers of every utterance scored as a batch of one (no padding: the masking modes coincide) ->
        list of dicts like ``evaluate_batch``'s.  ``texts``: list of (T_b,) ids without <eos>, ``speech``: list of
        (L_b, odim).  One ragged teacher-forced pass and one call per sum; an utterance's numbers are the same bits in any
        batch."""
        from .losses import bce_with_logits_sums, guided_attention_sums, pair_loss_sums
        if loss_type not in ("L1", "L2", "L1+L2"):
            raise ValueError("unknown --loss-type " + str(loss_type))
        guided = self._guided_setup(use_guided_attn_loss, modules_applied_guided_attn)
        ctx = Context.get(self._ctx.device)
        outs = self.teacher_forced_batch(texts, speech, seeds, spembs, guided, False)
        before, logits = self._read_teacher()
        L = np.asarray(self._last_frames, np.int64)              # (L_b // r) * r: ys is cut to it (:444-448)
        T = np.asarray(self._last_tok, np.int64)
        ys = torch.cat([ctx.to_device(y)[:int(n)] for y, n in zip(speech, L)])
        after = torch.cat([mel.as_subclass(torch.Tensor) for mel, _ in outs])
        sa, sb = pair_loss_sums(after, ys, L), pair_loss_sums(before, ys, L)
        n = L.astype(np.float64) * self.odim
        l1, l2 = (sa[:, 0] + sb[:, 0]) / n, (sa[:, 1] + sb[:, 1]) / n
        labels = torch.zeros(int(L.sum()), device=ctx.device)    # one utterance: only its last frame is 1
        labels[torch.as_tensor(np.cumsum(L) - 1, device=ctx.device)] = 1.0
        bce = bce_with_logits_sums(logits, labels, L, bce_pos_weight) / L
        res = {"bce_loss": bce, "l1_loss": l1, "l2_loss": l2}
        loss = {"L1": l1, "L2": l2, "L1+L2": l1 + l2}[loss_type] + bce
        if guided:
            maps = [self._selected_maps(a, 1) for _, a in outs]
            G = int(maps[0].shape[0])
            sums = guided_attention_sums(torch.cat([m.reshape(-1) for m in maps]), L, T, guided_attn_loss_sigma, maps=G)
            res["enc_dec_attn_loss"] = guided_attn_loss_lambda * sums[:, 0] / (G * L * T).astype(np.float64)
            loss = loss + res["enc_dec_attn_loss"]
        res["loss"] = loss
        alphas = self._alpha_entries()
        return [dict({k: float(v[b]) for k, v in res.items() if k != "loss"}, **alphas, loss=float(loss[b]))
                for b in range(len(outs))]

    def inference(self, text, speech=None, spembs=None, threshold=0.5, minlenratio=0.0, maxlenratio=10.0,
                  use_teacher_forcing=False, seed=0, denormalize=False):
        """(T,) int64 -> (outs (L, odim), probs (L,), att_ws (#layers, #heads, L, T + 1)); transformer_tts.py:511-647.
        With ``use_teacher_forcing``: (outs ((L // r) * r, odim), None, att_ws (#layers, #heads, L // r, T + 1)) for the
        teacher spectrogram ``speech`` (L, odim) (:567-579)."""
        if use_teacher_forcing:
            assert speech is not None, "speech must be provided with teacher forcing."   # :569
            outs, att = self.teacher_forced_batch([text], [speech], [seed], None if spembs is None else
                                                  to_numpy_f32(spembs).reshape(1, -1), True, denormalize)[0]
            return outs, None, att
        # ``speech`` feeds teacher forcing and the style encoder (:552-588); ignored otherwise
        return self.inference_batch([text], threshold, minlenratio, maxlenratio, [seed], True, denormalize,
                                    None if spembs is None else to_numpy_f32(spembs).reshape(1, -1),
                                    None if (speech is None or not self.use_gst) else [speech])[0]

    def debug_tap(self, what, b):
        """0: encoder output (T_b + 1, adim); 1: outs before the postnet (L_b, odim); 2: last decoder layer (L_b, adim)."""
        rows = (self._last_tok[b] if what == 0 else self._last_frames[b] if what == 1
                else self._last_frames[b] // self.reduction_factor)
        out = np.empty((rows, self.odim if what == 1 else self._adim), dtype=np.float32)
        _capi.check(self._ctx.lib.pk_tts_debug_read(self._h, what, b, _capi.fptr(out), out.size))
        return out


class TransformerTTSInference:
    """TransformerTTSInference (transformer_tts.py:757-767): inference()[0] then normalizer.inverse."""

    def __init__(self, normalizer, model):
        self.normalizer = normalizer
        self.acoustic_model = model
        self.bind()

    def bind(self):
        m = self.acoustic_model
        if getattr(m, "_norm_owner", None) is not self:
            m.set_normalizer(self.normalizer)
            m._norm_owner = self
        return m

    def forward(self, text, spk_id=None, seed=0):
        return self.bind().inference(text, seed=seed, denormalize=True)[0]

    __call__ = forward

    def eval(self):
        return self


class TransformerTTSLoss:
    """transformer_tts.py:770-871: ``(after_outs, before_outs, logits, ys, labels, olens)`` -> ``(l1_loss, mse_loss,
    bce_loss)``, 0-d float32 device tensors; the L1 and MSE terms each sum the after- and before-postnet errors.
    ``use_masking``: means over the valid frames; neither flag: means over the padded rectangles as given;
    ``use_weighted_masking``: every utterance's sum divided by L_b * B * odim (L_b * B for the stop term).  The stop term is
    Paddle's BCE with logits under ``bce_pos_weight``.  The device leaves float64 sums per utterance (``pk_pair_loss_run``,
    ``pk_bce_logits_run``); the means are formed on the host."""

    def __init__(self, use_masking=True, use_weighted_masking=False, bce_pos_weight=5.0):
        from .losses import masking_mode
        self._mode = masking_mode(use_masking, use_weighted_masking)
        self.use_masking, self.use_weighted_masking = use_masking, use_weighted_masking
        self.bce_pos_weight = float(bce_pos_weight)

    def terms(self, after_outs, before_outs, logits, ys, labels, olens):
        """The three numbers in float64."""
        from .losses import masked_bce_mean, masked_pair_means
        a1, a2 = masked_pair_means(after_outs, ys, olens, self._mode)
        b1, b2 = masked_pair_means(before_outs, ys, olens, self._mode)
        return a1 + b1, a2 + b2, masked_bce_mean(logits, labels, olens, self._mode, self.bce_pos_weight)

    def forward(self, after_outs, before_outs, logits, ys, labels, olens):
        from .losses import scalar
        return tuple(scalar(v) for v in self.terms(after_outs, before_outs, logits, ys, labels, olens))

    __call__ = forward


class GuidedAttentionLoss:
    """transformer_tts.py:874-1035: ``alpha`` times the mean of guide * att_ws over the entries inside both lengths, the
    guide ``1 - exp(-(t / ilen - s / olen)^2 / (2 sigma^2))``.  ``att_ws`` (B, T_max_out, T_max_in).  The sums come from
    ``pk_guided_attn_run`` (the guide is never stored); the one mean over every valid entry of the batch is formed on the
    host: alpha * sum_b sum(W A) / sum_b (olen_b * ilen_b).  ``reset_always`` is accepted: no mask is cached."""

    def __init__(self, sigma=0.4, alpha=1.0, reset_always=True):
        self.sigma, self.alpha, self.reset_always = sigma, alpha, reset_always

    def term(self, att_ws, ilens, olens):
        from .losses import _lengths, padded_guided_sums
        a = att_ws.as_subclass(torch.Tensor) if isinstance(att_ws, torch.Tensor) else torch.as_tensor(np.asarray(att_ws))
        G = 1 if a.dim() == 3 else int(a.shape[1])
        il, ol = _lengths(ilens), _lengths(olens)
        sums = padded_guided_sums(a, ol, il, self.sigma)
        return self.alpha * float(sums[:, 0].sum()) / float((G * ol * il).sum())

    def forward(self, att_ws, ilens, olens):
        from .losses import scalar
        if len(att_ws.shape) != 3:
            raise ValueError(f"att_ws {tuple(att_ws.shape)}: expected (B, T_max_out, T_max_in)")
        return scalar(self.term(att_ws, ilens, olens))

    __call__ = forward

    @staticmethod
    def _make_guided_attention_mask(ilen, olen, sigma):
        """(olen, ilen) device tensor, in the reference's order of operations (:984-989)."""
        ctx = Context.get()
        grid_x, grid_y = torch.meshgrid(torch.arange(olen, device=ctx.device), torch.arange(ilen, device=ctx.device),
                                        indexing="ij")
        grid_x, grid_y = grid_x.to(torch.float32), grid_y.to(torch.float32)
        return wrap(1.0 - torch.exp(-((grid_y / ilen - grid_x / olen) ** 2) / (2 * (sigma ** 2))))


class GuidedMultiHeadAttentionLoss(GuidedAttentionLoss):
    """transformer_tts.py:1038-1082: the same for (B, H, T_max_out, T_max_in); every head is one more map under the same
    guide, and the mean runs over H * olen_b * ilen_b entries per utterance."""

    def forward(self, att_ws, ilens, olens):
        from .losses import scalar
        if len(att_ws.shape) != 4:
            raise ValueError(f"att_ws {tuple(att_ws.shape)}: expected (B, H, T_max_out, T_max_in)")
        return scalar(self.term(att_ws, ilens, olens))

    __call__ = forward
