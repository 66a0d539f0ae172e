"""Tacotron2 acoustic model behind the reference's Python API.

Mirrors parakeet/models/tacotron2.py: ``Tacotron2`` (constructor kwargs :626-649, ``set_state_dict``, ``eval``,
``infer`` :781-840 -> dict of mel_output / mel_outputs_postnet / alignments [/ stop_logits], ``forward`` :691-778 with
eval semantics: the teacher-forced pass that ground-truth-aligned mels, scoring and alignment extraction need).  All
arithmetic runs in libpk_synth.so (csrc/taco2.hip).  ``Tacotron2Loss`` (:886-982) reduces on the engine (csrc/seq_loss.hip),
``evaluate_batch`` is ``forward`` followed by it; gradients and training-time dropout are out of scope;
reduction_factor > 1 is refused (the reference's ``infer`` and ``forward`` cannot run it either: the postnet gets the
(B, T, d_mels * r) decoder output, :822-826, :762).

The decoder prenet keeps dropout on at inference (:76-79, training=True); the mask comes from the engine's
counter-based dropout stream (include/pk_synth.h), selected by ``seed=``.

Extensions (superset): ``infer_batch`` decodes a ragged batch in lockstep, every utterance with its own stop;
``teacher_forced_batch`` is ``forward`` for a ragged batch without padding.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, set_params, to_numpy_f32, wrap


def _ids(v):
    if hasattr(v, "numpy") and not isinstance(v, (np.ndarray, torch.Tensor)):
        v = v.numpy()
    return np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v).astype(np.int64)


class Tacotron2:
    def __init__(self, vocab_size, n_tones=None, d_mels=80, d_encoder=512, encoder_conv_layers=3, encoder_kernel_size=5,
                 d_prenet=256, d_attention_rnn=1024, d_decoder_rnn=1024, attention_filters=32, attention_kernel_size=31,
                 d_attention=128, d_postnet=512, postnet_kernel_size=5, postnet_conv_layers=5, reduction_factor=1,
                 p_encoder_dropout=0.5, p_prenet_dropout=0.5, p_attention_dropout=0.1, p_decoder_dropout=0.1,
                 p_postnet_dropout=0.5, d_global_condition=None, use_stop_token=False, device=None):
        self.toned = n_tones is not None
        self.d_mels, self.d_encoder = d_mels, d_encoder
        self.d_global_condition = int(d_global_condition or 0)
        self.use_stop_token = bool(use_stop_token)
        self.training = True
        self._ctx = Context.get(device)
        cfg = _capi.TacoCfg()
        cfg.vocab_size, cfg.n_tones = vocab_size, int(n_tones or 0)
        cfg.d_mels, cfg.reduction_factor = d_mels, reduction_factor
        cfg.d_encoder, cfg.encoder_conv_layers, cfg.encoder_kernel_size = d_encoder, encoder_conv_layers, encoder_kernel_size
        cfg.d_prenet, cfg.d_attention_rnn, cfg.d_decoder_rnn = d_prenet, d_attention_rnn, d_decoder_rnn
        cfg.d_attention, cfg.attention_filters = d_attention, attention_filters
        cfg.attention_kernel_size = attention_kernel_size
        cfg.d_postnet, cfg.postnet_kernel_size, cfg.postnet_conv_layers = d_postnet, postnet_kernel_size, postnet_conv_layers
        cfg.d_global_condition = int(d_global_condition or 0)
        cfg.use_stop_token = 1 if use_stop_token else 0
        cfg.p_prenet_dropout = float(p_prenet_dropout)
        h = C.c_void_p()
        _capi.check(self._ctx.lib.pk_taco_create(self._ctx.handle, C.byref(cfg), C.byref(h)))
        self._h = h
        self._finalized = False
        self._last_tok, self._last_frames = [], []

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._ctx.lib.pk_taco_destroy(h)
            except Exception:
                pass

    def set_state_dict(self, state_dict):
        set_params(self._ctx.lib.pk_taco_set_param, self._h, state_dict)
        self._finalized = False

    def eval(self):
        self.training = False
        return self

    def set_math(self, mode):
        """'f16x3' (default: split-fp16 MFMA GEMMs, fp32-equivalent error) or 'f32' (exact fp32 MFMA)."""
        _capi.check(self._ctx.lib.pk_taco_set_math(self._h, {"f32": 0, "f16x3": 1}[mode]))

    def set_dropout(self, on):
        """False switches the decoder prenet's dropout off (deterministic; not what the reference computes)."""
        _capi.check(self._ctx.lib.pk_taco_set_dropout(self._h, 1 if on else 0))

    def _finalize(self):
        if not self._finalized:
            _capi.check(self._ctx.lib.pk_taco_finalize(self._h))
            self._finalized = True

    def _pack(self, texts, tones, seeds, global_condition):
        """The host arguments shared by pk_taco_infer and pk_taco_teacher; registers the global condition."""
        ctx = Context.get(self._ctx.device)
        self._finalize()
        if global_condition is not None:
            g = to_numpy_f32(global_condition).reshape(len(texts), -1)
            if g.shape[1] != self.d_global_condition:
                raise ValueError(f"global_condition has {g.shape[1]} columns, the model was built with "
                                 f"d_global_condition={self.d_global_condition or None}")
            _capi.check(ctx.lib.pk_taco_set_global_condition(self._h, _capi.fptr(g), g.shape[0]))
        ids = [_ids(t).reshape(-1) for t in texts]
        B = len(ids)
        lens = np.array([len(i) for i in ids], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(ids))
        tflat = None
        if tones is not None:
            tn = [_ids(t).reshape(-1) for t in tones]
            assert [len(t) for t in tn] == [len(i) for i in ids], "one tone per token"
            tflat = np.ascontiguousarray(np.concatenate(tn))
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
            assert sd.size == B, "one dropout seed per utterance"
        i64p = C.POINTER(C.c_int64)
        return (ctx, B, lens, flat.ctypes.data_as(i64p), None if tflat is None else tflat.ctypes.data_as(i64p),
                None if sd is None else sd.ctypes.data_as(C.POINTER(C.c_uint64)), (flat, tflat, sd))

    def _read(self, ctx, lens, frames):
        """pk_taco_read of the last infer / teacher call -> list of dicts, one per utterance."""
        self._last_tok, self._last_frames = [int(v) for v in lens], [int(v) for v in frames]
        total = int(frames.sum())
        mel, post = ctx.empty((total, self.d_mels)), ctx.empty((total, self.d_mels))
        align = ctx.empty((int(sum(L * T for L, T in zip(self._last_frames, self._last_tok))),))
        stop = ctx.empty((total,)) if self.use_stop_token else None
        _capi.check(ctx.lib.pk_taco_read(self._h, dptr(mel), dptr(post), dptr(align),
                                         None if stop is None else dptr(stop), 0))
        outs, o, oa = [], 0, 0
        for L, T in zip(self._last_frames, self._last_tok):
            d = {"mel_output": wrap(mel[o:o + L]), "mel_outputs_postnet": wrap(post[o:o + L]),
                 "alignments": wrap(align[oa:oa + L * T].view(L, T))}
            if stop is not None:
                d["stop_logits"] = wrap(stop[o:o + L])
            outs.append(d)
            o += L
            oa += L * T
        return outs

    def infer_batch(self, texts, max_decoder_steps=1000, tones=None, seeds=None, global_condition=None):
        """Lists of (T_b,) ids (and tone ids) -> list of dicts like ``infer`` returns, without the batch axis.
        ``global_condition``: (B, d_global_condition), one row per utterance (:816-821)."""
        ctx, B, lens, ids_p, tones_p, seeds_p, _keep = self._pack(texts, tones, seeds, global_condition)
        frames = np.zeros(B, dtype=np.int32)
        _capi.check(ctx.lib.pk_taco_infer(self._h, ids_p, tones_p, lens.ctypes.data_as(C.POINTER(C.c_int32)), B,
                                          int(max_decoder_steps), seeds_p, 0, frames.ctypes.data_as(C.POINTER(C.c_int32))))
        return self._read(ctx, lens, frames)

    def teacher_forced_batch(self, texts, mels, tones=None, seeds=None, global_condition=None):
        """The decoder teacher-forced on given mels (``Tacotron2Decoder.forward`` :419-472, eval semantics): lists of (T_b,)
        ids and of (L_b, d_mels) frames in the model's own mel domain, L_b >= 1 -> list of dicts with the keys of
        ``infer_batch``: mel_output (L_b, d_mels), mel_outputs_postnet, alignments (L_b, T_b) and, with a stop token,
        stop_logits (L_b,).  The query of step s is frame s - 1 of ``mels`` (zeros for s = 0); the decoder runs exactly L_b
        steps, a stop token ends nothing.  The prenet's dropout stays on, ``seeds`` as in ``infer_batch``: the teacher-forced
        pass on ``infer_batch``'s own mel_output with the same seeds returns ``infer_batch``'s outputs bit for bit."""
        if len(mels) != len(texts):
            raise ValueError(f"{len(texts)} texts but {len(mels)} teacher mels")
        dev = all(isinstance(m, torch.Tensor) and m.is_cuda for m in mels)
        rows = [m.detach().to(torch.float32) if dev else to_numpy_f32(m) for m in mels]
        for b, m in enumerate(rows):
            if m.ndim != 2 or m.shape[1] != self.d_mels:
                raise ValueError(f"teacher mel {b} has shape {tuple(m.shape)}, expected (L, {self.d_mels})")
            if m.shape[0] < 1:
                raise ValueError(f"teacher mel {b} is empty")
        ctx, B, lens, ids_p, tones_p, seeds_p, _keep = self._pack(texts, tones, seeds, global_condition)
        flens = np.array([m.shape[0] for m in rows], dtype=np.int32)
        if dev:
            packed = torch.cat(rows, dim=0).contiguous()
            mel_p, flags = dptr(packed), 0
        else:
            packed = np.ascontiguousarray(np.concatenate(rows, axis=0))
            mel_p, flags = _capi.fptr(packed), _capi.PK_HOST_IO
        frames = np.zeros(B, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        _capi.check(ctx.lib.pk_taco_teacher(self._h, ids_p, tones_p, lens.ctypes.data_as(i32p), B, mel_p,
                                            flens.ctypes.data_as(i32p), seeds_p, flags, frames.ctypes.data_as(i32p)))
        return self._read(ctx, lens, frames)

    def durations_batch(self, texts, mels, tones=None, seeds=None, global_condition=None, return_focus=False):
        """Token durations from the teacher-forced attention: ``teacher_forced_batch`` with these arguments,
        then ``alignment.durations_from_attention`` on its (L_b, T_b) alignments, which never leave the device.  Returns
        ``(durations, score)``: a list of (T_b,) int32 numpy arrays, each entry >= 1 and each array summing to L_b, and the (B,)
        float64 path scores (the sum of log attention along the path); with ``return_focus`` also the (B,) float64 focus
        rates of the alignments (``alignment.focus_rate``).  Needs T_b <= L_b.  These are the attention's boundaries, not a
        forced aligner's."""
        from .alignment import durations_from_attention, focus_rate
        outs = self.teacher_forced_batch(texts, mels, tones=tones, seeds=seeds, global_condition=global_condition)
        maps = [o["alignments"] for o in outs]
        res = durations_from_attention(maps)
        return res + (np.array([float(f) for f in focus_rate(maps)]),) if return_focus else res

    def forward(self, text_inputs, text_lens, mels, output_lens=None, tones=None, global_condition=None, seed=0):
        """``Tacotron2.forward`` (:691-778) with eval semantics (like ``infer``: only the prenet's dropout is live, stream
        ``seed + b`` for utterance b): text_inputs (B, T_text) padded ids, text_lens (B,), mels (B, T_mel, d_mels) padded,
        output_lens (B,) or None (every utterance has T_mel frames), tones (B, T_text) ->
        {"mel_output": (B, T_mel, d_mels), "mel_outputs_postnet": (B, T_mel, d_mels), "alignments": (B, T_mel, T_text),
        "stop_logits": (B, T_mel) with a stop token}.

        Every utterance is computed on its own text_lens[b] tokens and output_lens[b] frames; rows at or past output_lens[b]
        (and alignment columns at or past text_lens[b]) are zero.  For B = 1 and for a batch of equal lengths this is what
        the reference computes.  On a ragged padded batch the reference differs: its encoder convolutions are not masked
        (:233-237), so padded token rows leak into the valid ones next to them; the postnet is applied before the output mask
        (:762-769), so frames past output_lens[b] leak into the last valid ones; and it decodes the padded frames too, so its
        alignments and stop logits past output_lens[b] are not zero."""
        x = _ids(text_inputs)
        if x.ndim == 1:
            x = x[None]
        B = x.shape[0]
        tl = _ids(text_lens).reshape(-1)
        m = mels if isinstance(mels, torch.Tensor) and mels.is_cuda else to_numpy_f32(mels)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[0] != B or tl.size != B:
            raise ValueError(f"forward: {B} texts, {tl.size} text_lens, mels of shape {tuple(m.shape)}")
        T_mel = int(m.shape[1])
        ol = np.full(B, T_mel, dtype=np.int64) if output_lens is None else _ids(output_lens).reshape(-1)
        if ol.size != B or (ol < 1).any() or (ol > T_mel).any() or (tl < 1).any() or (tl > x.shape[1]).any():
            raise ValueError("forward: text_lens / output_lens out of range")
        tn = None
        if tones is not None:
            tn = _ids(tones).reshape(B, -1)
            tn = [tn[b, :tl[b]] for b in range(B)]
        outs = self.teacher_forced_batch([x[b, :tl[b]] for b in range(B)], [m[b, :ol[b]] for b in range(B)], tones=tn,
                                         seeds=[int(seed) + b for b in range(B)], global_condition=global_condition)
        ctx = Context.get(self._ctx.device)
        res = {"mel_output": torch.zeros((B, T_mel, self.d_mels), device=ctx.device),
               "mel_outputs_postnet": torch.zeros((B, T_mel, self.d_mels), device=ctx.device),
               "alignments": torch.zeros((B, T_mel, x.shape[1]), device=ctx.device)}
        if self.use_stop_token:
            res["stop_logits"] = torch.zeros((B, T_mel), device=ctx.device)
        for b, o in enumerate(outs):
            L, T = int(ol[b]), int(tl[b])
            res["mel_output"][b, :L] = o["mel_output"]
            res["mel_outputs_postnet"][b, :L] = o["mel_outputs_postnet"]
            res["alignments"][b, :L, :T] = o["alignments"]
            if self.use_stop_token:
                res["stop_logits"][b, :L] = o["stop_logits"]
        return {k: wrap(v) for k, v in res.items()}

    def evaluate_batch(self, text_inputs, text_lens, mels, output_lens, tones=None, global_condition=None, seed=0,
                       use_stop_token_loss=True, use_guided_attention_loss=False, sigma=0.2):
        """``forward`` on one padded batch, then ``Tacotron2Loss`` with the given options -> its dict as Python floats
        (``loss``, ``mel_loss``, ``post_mel_loss`` and, where selected, ``guided_attn_loss`` / ``stop_loss``).  The MSE terms
        and the stop loss are means over the whole padded rectangle, as in the reference.  On a ragged batch the engine's
        rows past output_lens[b] are zeros (see ``forward``), where the reference decodes the padding: its padded mel rows,
        and its padded stop logits in particular, are not zero, so the rectangle means differ there; for B = 1 and for equal
        lengths they are the reference's."""
        if use_stop_token_loss and not self.use_stop_token:
            raise ValueError("use_stop_token_loss needs a model built with use_stop_token=True")
        out = self.forward(text_inputs, text_lens, mels, output_lens, tones=tones, global_condition=global_condition, seed=seed)
        B, T_mel = out["mel_output"].shape[:2]
        ol = np.full(B, T_mel, dtype=np.int64) if output_lens is None else _ids(output_lens).reshape(-1)
        crit = Tacotron2Loss(use_stop_token_loss, use_guided_attention_loss, sigma)
        return {k: float(v) for k, v in crit.terms(out["mel_output"], out["mel_outputs_postnet"], mels, out["alignments"],
                                                   ol, _ids(text_lens).reshape(-1), out.get("stop_logits")).items()}

    def evaluate_per_utterance(self, texts, mels, tones=None, seeds=None, global_condition=None, use_stop_token_loss=True,
                               use_guided_attention_loss=False, sigma=0.2):
        """The criterion's numbers of every utterance scored as a batch of one -> list of dicts of Python floats.  Built on
        ``teacher_forced_batch`` (one ragged pass, no padding); the sums come from one call per term over the packed
        outputs, so an utterance's numbers are the same bits in any batch."""
        from .losses import bce_with_logits_sums, guided_attention_sums, pair_loss_sums
        if use_stop_token_loss and not self.use_stop_token:
            raise ValueError("use_stop_token_loss needs a model built with use_stop_token=True")
        ctx = Context.get(self._ctx.device)
        outs = self.teacher_forced_batch(texts, mels, tones=tones, seeds=seeds, global_condition=global_condition)
        L, T = np.asarray(self._last_frames, np.int64), np.asarray(self._last_tok, np.int64)
        cat = lambda key: torch.cat([o[key].as_subclass(torch.Tensor).reshape(-1) for o in outs])   # noqa: E731
        ys = torch.cat([ctx.to_device(m).reshape(-1) for m in mels]).reshape(-1, self.d_mels)
        n = L.astype(np.float64) * self.d_mels
        res = {"mel_loss": pair_loss_sums(cat("mel_output").reshape(-1, self.d_mels), ys, L)[:, 1] / n,
               "post_mel_loss": pair_loss_sums(cat("mel_outputs_postnet").reshape(-1, self.d_mels), ys, L)[:, 1] / n}
        total = res["mel_loss"] + res["post_mel_loss"]
        if use_guided_attention_loss:
            res["guided_attn_loss"] = guided_attention_sums(cat("alignments"), L, T, sigma)[:, 0] / (L * T)
            total = total + res["guided_attn_loss"]
        if use_stop_token_loss:
            labels = torch.zeros(int(L.sum()), device=ctx.device)
            labels[torch.as_tensor(np.cumsum(L) - 1, device=ctx.device)] = 1.0
            res["stop_loss"] = bce_with_logits_sums(cat("stop_logits"), labels, L) / L
            total = total + res["stop_loss"]
        res["loss"] = total
        return [{k: float(v[b]) for k, v in res.items()} for b in range(len(outs))]

    def infer(self, text_inputs, max_decoder_steps=1000, tones=None, global_condition=None, seed=0):
        """text_inputs (1, T) [or (T,)] int64 -> {"mel_output": (1, L, C), "mel_outputs_postnet": (1, L, C),
        "alignments": (1, L, T), "stop_logits": (1, L) with a stop token}; tacotron2.py:781-840."""
        x = _ids(text_inputs)
        if x.ndim == 2 and x.shape[0] != 1:
            raise ValueError("infer() takes one utterance (the reference's stop test needs batch size 1, "
                             "tacotron2.py:515-521); use infer_batch for several")
        t = None if tones is None else [_ids(tones).reshape(-1)]
        o = self.infer_batch([x.reshape(-1)], max_decoder_steps, t, [seed], global_condition)[0]
        return {k: wrap(v.unsqueeze(0)) for k, v in o.items()}

    @classmethod
    def from_pretrained(cls, config, checkpoint_path):
        """Tacotron2.from_pretrained (tacotron2.py:843-883): config with ``model`` / ``data`` sections, checkpoint path
        without the ``.pdparams`` suffix."""
        from .checkpoint import load_tacotron2
        return load_tacotron2(config, checkpoint_path)

    def debug_tap(self, what, b):
        """0: encoder outputs (T_b, d_encoder)."""
        out = np.empty((self._last_tok[b], self.d_encoder), dtype=np.float32)
        _capi.check(self._ctx.lib.pk_taco_debug_read(self._h, what, b, _capi.fptr(out), out.size))
        return out


class Tacotron2Loss:
    """tacotron2.py:886-982 -> the reference's dict of 0-d float32 device tensors: ``loss``, ``mel_loss``,
    ``post_mel_loss`` and, where selected, ``guided_attn_loss`` (``guided_attention_loss`` of modules/losses.py under
    ``sigma``) and ``stop_loss``.  The MSE terms are means over the whole rectangle given; the stop labels are
    ``one_hot(slens - 1, T_dec)`` and the BCE a mean over all B * T_dec logits (:960-971).  The device leaves float64 sums
    (``pk_pair_loss_run``, ``pk_bce_logits_run``, ``pk_guided_attn_run``); means and the total are formed on the host."""

    def __init__(self, use_stop_token_loss=True, use_guided_attention_loss=False, sigma=0.2):
        self.use_stop_token_loss = use_stop_token_loss
        self.use_guided_attention_loss = use_guided_attention_loss
        self.sigma = sigma

    def terms(self, mel_outputs, mel_outputs_postnet, mel_targets, attention_weights=None, slens=None, plens=None,
              stop_logits=None):
        """The dict in float64."""
        from .losses import _lengths, masked_bce_mean, masked_pair_means, padded_guided_sums
        ctx = Context.get()
        mel_loss = masked_pair_means(mel_outputs, mel_targets, None, "none")[1]
        post = masked_pair_means(mel_outputs_postnet, mel_targets, None, "none")[1]
        losses = {"loss": mel_loss + post, "mel_loss": mel_loss, "post_mel_loss": post}
        if self.use_guided_attention_loss:
            if attention_weights is None or slens is None or plens is None:
                raise ValueError("the guided attention loss needs attention_weights, slens and plens")
            dl, el = _lengths(slens), _lengths(plens)
            sums = padded_guided_sums(attention_weights, dl, el, self.sigma)
            losses["guided_attn_loss"] = float(np.mean(sums[:, 0] / (dl * el).astype(np.float64)))
            losses["loss"] += losses["guided_attn_loss"]
        if self.use_stop_token_loss:
            if stop_logits is None or slens is None:
                raise ValueError("the stop token loss needs stop_logits and slens")
            x = ctx.to_device(stop_logits)
            sl = torch.as_tensor(_lengths(slens), device=ctx.device)
            if x.dim() != 2 or sl.numel() != x.shape[0] or int(sl.min()) < 1 or int(sl.max()) > x.shape[1]:
                raise ValueError(f"stop_logits {tuple(x.shape)} with slens {sl.tolist()}")
            labels = torch.zeros_like(x)
            labels[torch.arange(x.shape[0], device=ctx.device), sl - 1] = 1.0
            losses["stop_loss"] = masked_bce_mean(x, labels, None, "none")
            losses["loss"] += losses["stop_loss"]
        return losses

    def forward(self, mel_outputs, mel_outputs_postnet, mel_targets, attention_weights=None, slens=None, plens=None,
                stop_logits=None):
        from .losses import scalar
        return {k: scalar(v) for k, v in self.terms(mel_outputs, mel_outputs_postnet, mel_targets, attention_weights, slens,
                                                    plens, stop_logits).items()}

    __call__ = forward
