"""``parakeet/modules/losses.py`` on the HIP engine, and the per-utterance sums behind the evaluators' criteria.

``weighted_mean`` (:60-77) and ``masked_l1_loss`` (:80-100) run on ``pk_mel_loss_run`` (csrc/mel_loss.hip: masked L1 and SSIM
of mel pairs in one pass; ``mel_loss_sums`` and ``parakeet_amd.ssim`` expose its sums).  ``attention_guide`` (:26-47) and
``guided_attention_loss`` (:50-57) are here too, the loss on ``pk_guided_attn_run``.  ``pair_loss_sums``,
``bce_with_logits_sums`` and ``guided_attention_sums`` (csrc/seq_loss.hip) are what ``FastSpeech2Loss``,
``TransformerTTSLoss``, ``GuidedAttentionLoss`` and ``Tacotron2Loss`` (in their models' modules) reduce: float64 sums per
utterance from the device, means formed on the host.  ``pwg_evaluate`` forms the seven numbers of the Parallel WaveGAN
evaluator.  ``masked_softmax_with_cross_entropy`` (:103-127) is not implemented: no model on the engine uses it.  Inference
only: no gradients."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, wrap

__all__ = ["weighted_mean", "masked_l1_loss", "mel_loss_sums", "pair_loss_sums", "bce_with_logits_sums",
           "guided_attention_sums", "attention_guide", "guided_attention_loss", "pwg_evaluate", "pwg_evaluate_per_utterance"]


def _t(x):
    return (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).as_subclass(torch.Tensor)


def mel_loss_sums(pred, target, lens, padded=None, window_size=11, return_map=False):
    """``pk_mel_loss_run``.  pred, target: packed rows (sum(lens), W); lens: rows of each pair; padded: rows of each pair's
    SSIM map (>= lens; the rows past lens read as zero in both images), default lens.  Returns (B, 2) float64 numpy: sum
    |pred - target| over each pair's entries, sum of its SSIM map; with ``return_map`` also the packed (sum(padded), W) map
    as a device tensor."""
    ctx = Context.get()
    lens = np.ascontiguousarray(np.asarray(lens).reshape(-1), dtype=np.int32)
    pl = None if padded is None else np.ascontiguousarray(np.asarray(padded).reshape(-1), dtype=np.int32)
    B = int(lens.size)
    if B == 0:
        raise ValueError("no pairs given")
    if pl is not None and pl.size != B:
        raise ValueError(f"{B} pairs, {pl.size} padded lengths")
    p, t = ctx.to_device(pred), ctx.to_device(target)
    if p.dim() != 2 or p.shape != t.shape:
        raise ValueError(f"prediction {tuple(p.shape)} against target {tuple(t.shape)}: both must be (rows, W)")
    if p.shape[0] != int(lens.sum()):
        raise ValueError(f"{p.shape[0]} packed rows, the lengths sum to {int(lens.sum())}")
    W = int(p.shape[1])
    i32p = C.POINTER(C.c_int32)
    out = ctx.empty((B, 2), dtype=torch.float64)
    ssim_map = ctx.empty((int((lens if pl is None else pl).sum()), W)) if return_map else None
    _capi.check(ctx.lib.pk_mel_loss_run(ctx.handle, dptr(p), dptr(t), lens.ctypes.data_as(i32p),
                                        None if pl is None else pl.ctypes.data_as(i32p), B, W, int(window_size), dptr(out),
                                        None if ssim_map is None else dptr(ssim_map), 0))
    sums = out.cpu().numpy()
    return (sums, ssim_map) if return_map else sums


def _i32(x):
    return np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int32)


def _i64(x):
    return None if x is None else np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int64)


def _p(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _lengths(x):
    """Lengths given as a list, numpy or a tensor on any device -> (B,) int64 numpy."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().as_subclass(torch.Tensor).numpy()
    return np.asarray(x).reshape(-1).astype(np.int64)


def scalar(value, ctx=None):
    """A float64 host number -> the 0-d float32 device tensor the criteria return."""
    ctx = ctx or Context.get()
    return wrap(torch.tensor(float(value), dtype=torch.float32, device=ctx.device))


def _extent_check(name, numel, offs, span):
    if offs is None:
        need = int(span.sum())
    else:
        if (offs < 0).any():
            raise ValueError(f"{name}: negative offset")
        need = int((offs + span).max()) if span.size else 0
    if need > numel:
        raise ValueError(f"{name}: the layout reaches entry {need} of a tensor of {numel}")


def pair_loss_sums(pred, target, rows, pred_offsets=None, target_offsets=None, pred_stride=0, target_stride=0, width=None):
    """``pk_pair_loss_run``.  pred, target: float32 numpy or device tensors; pair b is ``rows[b]`` x W entries of each, row r
    of the prediction at flat index ``pred_offsets[b] + r * pred_stride`` (target likewise).  Without offsets the pairs are
    packed, (sum(rows), W) or, for W = 1, (sum(rows),).  W is ``width`` or the operands' last dimension; a stride of 0
    means W.  A padded (B, Lmax, W) rectangle is ``offsets = arange(B) * Lmax * W``.  Returns (B, 2) float64 numpy: sum
    |pred - target| and sum (pred - target)^2 over each pair's entries."""
    ctx = Context.get()
    rows = _i32(rows)
    B = int(rows.size)
    if B == 0:
        raise ValueError("no pairs given")
    p, t = ctx.to_device(pred), ctx.to_device(target)
    W = int(width) if width is not None else (int(p.shape[-1]) if p.dim() >= 2 else 1)
    po, to = _i64(pred_offsets), _i64(target_offsets)
    for name, x, o, st in (("pred", p, po, pred_stride), ("target", t, to, target_stride)):
        if o is not None and o.size != B:
            raise ValueError(f"{B} pairs, {o.size} {name} offsets")
        st = int(st) or W
        r64 = rows.astype(np.int64)
        _extent_check(name, x.numel(), o, np.where(r64 > 0, (r64 - 1) * st + W, 0) if o is not None else r64 * W)
    out = ctx.empty((B, 2), dtype=torch.float64)
    _capi.check(ctx.lib.pk_pair_loss_run(ctx.handle, dptr(p), dptr(t), _p(po, C.c_int64), _p(to, C.c_int64), int(pred_stride),
                                         int(target_stride), _p(rows, C.c_int32), B, W, dptr(out), 0))
    return out.cpu().numpy()


def bce_with_logits_sums(logits, labels, lens, pos_weight=1.0, logit_offsets=None, label_offsets=None):
    """``pk_bce_logits_run``.  Row b is ``lens[b]`` float32 logits x and float labels y at the given flat offsets (default:
    packed).  Returns (B,) float64 numpy: the sum over each row of Paddle's ``binary_cross_entropy_with_logits`` term
    ``(1 - y) x + (1 + (pos_weight - 1) y) (log1p(exp(-|x|)) + max(-x, 0))``."""
    ctx = Context.get()
    lens = _i32(lens)
    B = int(lens.size)
    if B == 0:
        raise ValueError("no rows given")
    x, y = ctx.to_device(logits), ctx.to_device(labels)
    xo, yo = _i64(logit_offsets), _i64(label_offsets)
    for name, v, o in (("logits", x, xo), ("labels", y, yo)):
        if o is not None and o.size != B:
            raise ValueError(f"{B} rows, {o.size} {name} offsets")
        _extent_check(name, v.numel(), o, lens.astype(np.int64))
    out = ctx.empty((B,), dtype=torch.float64)
    _capi.check(ctx.lib.pk_bce_logits_run(ctx.handle, dptr(x), dptr(y), _p(xo, C.c_int64), _p(yo, C.c_int64),
                                          _p(lens, C.c_int32), B, float(pos_weight), dptr(out), 0))
    return out.cpu().numpy()


def guided_attention_sums(att, rows, cols, sigma, maps=1, offsets=None, map_stride=0, row_stride=0):
    """``pk_guided_attn_run``.  Utterance b owns ``maps[b]`` (an int: the same for all) attention maps of ``rows[b]`` x
    ``cols[b]`` float32 entries; map g's row s lies at flat index ``offsets[b] + g * map_stride + s * row_stride`` of
    ``att``.  Without offsets everything is contiguous, utterance after utterance.  A zero-padded (B, G, Smax, Tmax) tensor
    is ``offsets = arange(B) * G * Smax * Tmax, map_stride = Smax * Tmax, row_stride = Tmax``.  Returns (B, 2) float64
    numpy: sum of W * A under the guide ``W[s, t] = 1 - exp(-(t / cols[b] - s / rows[b])^2 / (2 sigma^2))``, and sum of
    A."""
    ctx = Context.get()
    rows, cols = _i32(rows), _i32(cols)
    B = int(rows.size)
    if B == 0:
        raise ValueError("no utterances given")
    maps = np.full(B, int(maps), dtype=np.int32) if np.ndim(maps) == 0 else _i32(maps)
    if cols.size != B or maps.size != B:
        raise ValueError(f"{B} row counts, {cols.size} column counts, {maps.size} map counts")
    a = ctx.to_device(att)
    offs = _i64(offsets)
    if offs is not None and offs.size != B:
        raise ValueError(f"{B} utterances, {offs.size} offsets")
    r64, c64, g64 = rows.astype(np.int64), cols.astype(np.int64), maps.astype(np.int64)
    ss = np.full(B, int(row_stride), np.int64) if row_stride else c64
    gs = np.full(B, int(map_stride), np.int64) if map_stride else r64 * ss
    _extent_check("att", a.numel(), offs, g64 * gs if offs is None else (g64 - 1) * gs + (r64 - 1) * ss + c64)
    out = ctx.empty((B, 2), dtype=torch.float64)
    _capi.check(ctx.lib.pk_guided_attn_run(ctx.handle, dptr(a), _p(offs, C.c_int64), int(map_stride), int(row_stride),
                                           _p(maps, C.c_int32), _p(rows, C.c_int32), _p(cols, C.c_int32), B, float(sigma),
                                           dptr(out), 0))
    return out.cpu().numpy()


def padded_guided_sums(att_ws, rows, cols, sigma):
    """``guided_attention_sums`` of a zero-padded (B, Smax, Tmax) or (B, G, Smax, Tmax) tensor."""
    a = Context.get().to_device(att_ws)
    if a.dim() == 3:
        a = a.unsqueeze(1)
    if a.dim() != 4:
        raise ValueError(f"attention weights {tuple(a.shape)}: expected (B, T_out, T_in) or (B, H, T_out, T_in)")
    B, G, S, T = a.shape
    rows, cols = _lengths(rows), _lengths(cols)
    if rows.size != B or cols.size != B:
        raise ValueError(f"{B} utterances, {rows.size} and {cols.size} lengths")
    if (rows > S).any() or (cols > T).any():
        raise ValueError(f"lengths {rows.tolist()} x {cols.tolist()} exceed the maps' {S} x {T}")
    return guided_attention_sums(a, rows, cols, sigma, maps=G, offsets=np.arange(B, dtype=np.int64) * (G * S * T),
                                 map_stride=S * T, row_stride=T)


def attention_guide(dec_lens, enc_lens, N, T, g, dtype=None):
    """losses.py:26-47: ``W[i, n, t] = 1 - exp(-(n / dec_lens[i] - t / enc_lens[i])^2 / (2 g^2))`` under the two length
    masks, materialised as a (B, N, T) device tensor in the reference's order of operations (plain tensor ops: the loss
    below never stores it)."""
    ctx = Context.get()
    dtype = dtype or torch.float32
    dl = torch.as_tensor(_lengths(dec_lens), device=ctx.device)
    el = torch.as_tensor(_lengths(enc_lens), device=ctx.device)
    dec_pos = torch.arange(0, N, device=ctx.device).to(dtype) / dl.unsqueeze(-1)
    enc_pos = torch.arange(0, T, device=ctx.device).to(dtype) / el.unsqueeze(-1)
    W = 1 - torch.exp(-(dec_pos.unsqueeze(-1) - enc_pos.unsqueeze(1)) ** 2 / (2 * g ** 2))
    mask = (torch.arange(N, device=ctx.device)[None, :] < dl[:, None]).unsqueeze(-1) \
        & (torch.arange(T, device=ctx.device)[None, :] < el[:, None]).unsqueeze(1)
    return wrap(W * mask.to(W.dtype))


def guided_attention_loss(attention_weight, dec_lens, enc_lens, g):
    """losses.py:50-57 for (B, T_dec, T_enc) attention weights: the mean over b of sum(W_b * A_b) / (dec_len_b *
    enc_len_b), the sums from ``pk_guided_attn_run``, the quotients and the mean in float64 on the host.  Returns a 0-d
    float32 device tensor."""
    dl, el = _lengths(dec_lens), _lengths(enc_lens)
    sums = padded_guided_sums(attention_weight, dl, el, g)
    return scalar(np.mean(sums[:, 0] / (dl * el).astype(np.float64)))


def masking_mode(use_masking, use_weighted_masking):
    """The flag pair of FastSpeech2Loss / TransformerTTSLoss (with the reference's assertion) -> "mask", "weighted", "none"."""
    assert (use_masking != use_weighted_masking) or not use_masking
    return "mask" if use_masking else "weighted" if use_weighted_masking else "none"


def _rect3(x, ctx):
    t = ctx.to_device(x)
    return t.unsqueeze(-1) if t.dim() == 2 else t


def masked_pair_means(pred, target, lens, mode):
    """L1 and MSE of padded (B, Lmax, W) or (B, Lmax) rectangles under a length mask, as nn.L1Loss / nn.MSELoss are used
    by FastSpeech2Loss and TransformerTTSLoss: ``mode`` "mask" is the mean over the valid entries, "none" the mean over the
    whole rectangle, "weighted" the sum over b of the valid entries' sum / (lens[b] * B * W).  One ``pk_pair_loss_run``
    over the rectangles in place.  Returns two float64 numbers."""
    ctx = Context.get()
    p, t = _rect3(pred, ctx), _rect3(target, ctx)
    if p.dim() != 3 or t.dim() != 3 or p.shape[0] != t.shape[0] or p.shape[2] != t.shape[2]:
        raise ValueError(f"prediction {tuple(p.shape)} against target {tuple(t.shape)}")
    B, Lp, W = p.shape
    Lt = int(t.shape[1])
    if mode == "none":
        if Lp != Lt:
            raise ValueError(f"prediction {tuple(p.shape)} against target {tuple(t.shape)}")
        rows = np.full(B, Lp, np.int64)
    else:
        rows = _lengths(lens)
        if rows.size != B or (rows < 0).any() or (rows > min(Lp, Lt)).any():
            raise ValueError(f"lengths {rows.tolist()} for rectangles of {Lp} and {Lt} rows")
    ar = np.arange(B, dtype=np.int64)
    sums = pair_loss_sums(p, t, rows, ar * (Lp * W), ar * (Lt * W), width=W)
    if mode == "weighted":
        n = rows.astype(np.float64) * (B * W)
        return float((sums[:, 0] / n).sum()), float((sums[:, 1] / n).sum())
    n = float(rows.sum()) * W
    return float(sums[:, 0].sum() / n), float(sums[:, 1].sum() / n)


def masked_bce_mean(logits, labels, lens, mode, pos_weight=1.0):
    """nn.BCEWithLogitsLoss of padded (B, Lmax) logits and labels under a length mask, modes as ``masked_pair_means``
    ("weighted": sum over b of the row's sum / (lens[b] * B)).  Returns a float64 number."""
    ctx = Context.get()
    x, y = ctx.to_device(logits), ctx.to_device(labels)
    if x.dim() != 2 or x.shape != y.shape:
        raise ValueError(f"logits {tuple(x.shape)} against labels {tuple(y.shape)}")
    B, L = x.shape
    if mode == "none":
        rows = np.full(B, L, np.int64)
    else:
        rows = _lengths(lens)
        if rows.size != B or (rows < 0).any() or (rows > L).any():
            raise ValueError(f"lengths {rows.tolist()} for {L} logits per row")
    offs = np.arange(B, dtype=np.int64) * L
    sums = bce_with_logits_sums(x, y, rows, pos_weight, offs, offs)
    if mode == "weighted":
        return float((sums / (rows.astype(np.float64) * B)).sum())
    return float(sums.sum() / float(rows.sum()))


def weighted_mean(input, weight):   # noqa: A002  (the reference's argument name)
    """losses.py:60-77: ``sum(input * weight) / (sum(weight) * input.size / weight.size)``, on the input's device."""
    x = _t(input)
    w = _t(weight).to(device=x.device, dtype=x.dtype)
    ratio = x.numel() / w.numel()
    return wrap(torch.sum(x * w) / (torch.sum(w) * ratio))


def _prefix_lengths(mask, B, L):
    """Lengths of a (B, L, 1) frame mask of prefix form (ones, then zeros), or None."""
    m = _t(mask)
    if tuple(m.shape) != (B, L, 1):
        return None
    m = m.detach().cpu().reshape(B, L).to(torch.float64).numpy()
    lens = m.sum(1).astype(np.int64)
    if not np.array_equal(m, (np.arange(L)[None, :] < lens[:, None]).astype(np.float64)):
        return None
    return lens


def masked_l1_loss(prediction, target, mask):
    """losses.py:80-100 for (B, L, D) spectrograms under a frame mask (B, L, 1) of prefix form, as
    ``F.sequence_mask(num_frames).unsqueeze(-1)`` is: the absolute error summed by ``pk_mel_loss_run`` over the valid frames,
    divided on the host in float64 by ``sum(mask) * D``.  Returns a 0-d float32 device tensor.

    An evaluator's call, not a training loop's: the mask is read on the host to find the lengths, and the pass is the
    L1 + SSIM pass at window 1 (its map, one multiply-divide per entry, is formed and dropped); there is no L1-only kernel."""
    p, t = _t(prediction), _t(target)
    if p.dim() != 3 or p.shape != t.shape:
        raise NotImplementedError(f"masked_l1_loss: prediction {tuple(p.shape)} and target {tuple(t.shape)} must be one "
                                  "(B, L, D) shape")
    B, L, D = p.shape
    lens = _prefix_lengths(mask, B, L)
    if lens is None:
        raise NotImplementedError("masked_l1_loss runs on the engine for a frame mask (B, L, 1) of prefix form; any other "
                                  "mask is not implemented")
    if lens.sum() == 0:
        raise ValueError("the mask selects no frame: there is nothing to average")
    ctx = Context.get()
    p, t = ctx.to_device(p), ctx.to_device(t)
    pack = lambda x: torch.cat([x[b, :int(lens[b])] for b in range(B)])   # noqa: E731
    sums = mel_loss_sums(pack(p), pack(t), lens, window_size=1)
    return wrap(torch.tensor(sums[:, 0].sum() / (float(lens.sum()) * D), dtype=torch.float32, device=ctx.device))


def _utterances(x):
    """(N, 1, T) or (N, T) -> list of N 1-D signals"""
    t = _t(x)
    if t.dim() == 3:
        t = t.reshape(-1, t.shape[2])
    if t.dim() != 2:
        raise AssertionError(f"expected (N, 1, T) or (N, T), got {tuple(t.shape)}")
    return [t[n] for n in range(t.shape[0])]


def _pwg_numbers(adv, real, fake, sc, mag, lambda_adv):
    return {"eval/adversarial_loss": adv, "eval/spectral_convergence_loss": sc, "eval/log_stft_magnitude_loss": mag,
            "eval/generator_loss": lambda_adv * adv + sc + mag, "eval/real_loss": real, "eval/fake_loss": fake,
            "eval/discriminator_loss": real + fake}


def pwg_evaluate(generator, discriminator, stft_criterion, wav, mel, noise, lambda_adv):
    """``PWGEvaluator.evaluate_core`` (parallel_wavegan_updater.py:180-231) for one rectangle: ``wav`` (N, 1, T) ground truth,
    ``mel`` (N, aux, T' + 2 ctx), ``noise`` (N, 1, T) in place of the ``paddle.randn`` drawn inside the call.  Returns the
    seven ``eval/*`` numbers as Python floats.  ``generator(noise, mel)`` is ``PWGGenerator.forward``;
    ``discriminator.scores`` gives the sums of (p - 1)^2 and p^2 per utterance, from which the three MSE terms are formed
    here in float64 as means over all N x T logits; ``stft_criterion(wav_, wav)`` is ``MultiResolutionSTFTLoss``."""
    wav_ = generator(noise, mel)
    s_fake, n_fake = discriminator.scores(_utterances(wav_))
    s_real, n_real = discriminator.scores(_utterances(wav))
    adv = float(s_fake[:, 0].sum() / n_fake.sum())
    fake = float(s_fake[:, 1].sum() / n_fake.sum())
    real = float(s_real[:, 0].sum() / n_real.sum())
    sc, mag = stft_criterion(wav_, wav)
    return _pwg_numbers(adv, real, fake, float(sc), float(mag), float(lambda_adv))


def pwg_evaluate_per_utterance(discriminator, stft_criterion, generated, real, lambda_adv):
    """The same seven numbers for a ragged corpus: ``generated`` and ``real`` are lists of 1-D signals, pairwise of equal
    length; every pair is scored as the evaluator would score a batch of one.  Returns ``{key: (B,) float64 numpy}``;
    ``stft_criterion.per_utterance`` supplies the two STFT losses, averaged over its resolutions."""
    generated, real = list(generated), list(real)
    s_fake, n_fake = discriminator.scores(generated)
    s_real, n_real = discriminator.scores(real)
    per = np.asarray(stft_criterion.per_utterance(generated, real), np.float64).mean(axis=1)   # (B, R, 2) -> (B, 2)
    return _pwg_numbers(s_fake[:, 0] / n_fake, s_real[:, 0] / n_real, s_fake[:, 1] / n_fake, per[:, 0], per[:, 1],
                        float(lambda_adv))
