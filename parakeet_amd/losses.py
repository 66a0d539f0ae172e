"""``parakeet/modules/losses.py``'s ``weighted_mean`` (:60-77) and ``masked_l1_loss`` (:80-100) on the HIP engine, and the
sums behind them and behind ``parakeet_amd.ssim`` (``pk_mel_loss_run``, csrc/mel_loss.hip: masked L1 and SSIM of mel pairs in
one pass).  ``pwg_evaluate`` forms the seven numbers of the Parallel WaveGAN evaluator.  ``guided_attention_loss`` and ``masked_softmax_with_cross_entropy`` are not implemented.  Inference only: no
gradients."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, wrap

__all__ = ["weighted_mean", "masked_l1_loss", "mel_loss_sums", "pwg_evaluate", "pwg_evaluate_per_utterance"]


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
