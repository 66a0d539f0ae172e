"""Scores of free-running synthesis: mel-cepstral distortion and log-F0 RMSE along a dynamic-time-warping
path, for synthesised signals whose lengths differ from the recordings'.

Everything here is this project's own definition and says so where it matters:
  * the cepstra are the orthonormal DCT-II of the natural-log mel spectrum the engine's ``LogMelFBank`` produces, NOT SPTK's
    ``mcep`` (no frequency warping, no spectral-envelope estimation);
  * the path is the unconstrained DTW of ``parakeet_amd.alignment`` (squared Euclidean local cost over c_1 ... c_n_coef, no
    band, no slope weights);
  * f0 and voicing are ``audio.Pitch``'s (this project's YIN-style estimator), not pyworld's.
Nobody has compared these numbers with another toolkit's on speech.

The warping, the sums along the path, the mel and f0 extraction and the DCT product run on the HIP engine; torch only moves
data and forms the logarithm / voicing mask of the f0 tracks."""
import math

import numpy as np
import torch

from . import _capi
from .alignment import dtw_features, path_stats
from .runtime import Context, dptr, wrap

__all__ = ["dct_matrix", "mel_cepstrum", "mcd_result", "f0_result", "mcd_batch", "f0_batch", "score_batch"]

_DCT = {}


def dct_matrix(n_mels, n_coef):
    """(n_mels, n_coef + 1) float64: column k is the orthonormal DCT-II basis vector k,
    w[n, k] = sqrt(2 / n_mels) cos(pi (n + 1/2) k / n_mels), column 0 sqrt(1 / n_mels)."""
    n_mels, n_coef = int(n_mels), int(n_coef)
    if n_mels < 1 or not 0 <= n_coef < n_mels:
        raise ValueError(f"n_coef = {n_coef} must lie in 0 ... n_mels - 1 = {n_mels - 1}")
    # the angle pi (2 n + 1) k / (2 n_mels) is reduced in integers to [0, pi / 2] before cos / sin see it: the entries are
    # then good to an ulp and the rows orthonormal to 1e-15 (a float64 angle of tens of radians costs ten times that)
    N4 = 4 * n_mels
    m = (2 * np.arange(n_mels, dtype=np.int64)[:, None] + 1) * np.arange(n_coef + 1, dtype=np.int64)[None, :] % N4
    m = np.where(m > 2 * n_mels, N4 - m, m)                # cos(2 pi - a) = cos a: now 0 <= a <= pi
    sign = np.where(m > n_mels, -1.0, 1.0)
    m = np.where(m > n_mels, 2 * n_mels - m, m)            # cos(pi - a) = -cos a: now 0 <= a <= pi / 2
    near = 2 * m <= n_mels
    c = np.where(near, np.cos(np.pi * m / (2.0 * n_mels)), np.sin(np.pi * (n_mels - m) / (2.0 * n_mels)))
    w = sign * c * np.sqrt(2.0 / n_mels)
    w[:, 0] = np.sqrt(1.0 / n_mels)
    return w


def _check_base(log_base):
    b = float(log_base)
    if not (b > 0 and b != 1 and math.isfinite(b)):
        raise ValueError(f"log_base = {log_base} must be a positive finite number other than 1")
    return b


def cepstrum_matrix(n_mels, n_coef, log_base=10.0):
    """The float32 (n_mels, n_coef + 1) matrix ``mel_cepstrum`` multiplies by: ln(log_base) * dct_matrix, built in float64 and
    rounded once (the change of the logarithm's base is folded into the matrix instead of rounding the log-mel once more)."""
    key = (int(n_mels), int(n_coef), _check_base(log_base))
    if key not in _DCT:
        _DCT[key] = np.ascontiguousarray((math.log(key[2]) * dct_matrix(n_mels, n_coef)).astype(np.float32))
    return _DCT[key]


def mel_cepstrum(logmel, n_coef=13, log_base=10.0):
    """c_0 ... c_n_coef of log-mel frames: the orthonormal DCT-II of the natural-log mel spectrum (``logmel`` is in base
    ``log_base``, as ``LogMelFBank`` returns it).  ``logmel``: one (frames, n_mels) array / tensor or a list of such; returns
    device tensors (frames, n_coef + 1), views of one packed tensor for a list.  The product runs on the engine's exact-fp32
    GEMM (``pk_op_matmul``).  This is NOT SPTK's mel-cepstrum."""
    single = hasattr(logmel, "shape")
    mels = [logmel] if single else list(logmel)
    if not mels:
        raise ValueError("no log-mel sequences given")
    for b, m in enumerate(mels):
        if not hasattr(m, "shape") or len(m.shape) != 2 or min(m.shape) < 1:
            raise ValueError(f"log-mel {b}: expected (frames, n_mels), got " + (f"shape {tuple(m.shape)}" if hasattr(m, "shape")
                                                                                 else type(m).__name__))
        if m.shape[1] != mels[0].shape[1]:
            raise ValueError(f"log-mel {b} has {int(m.shape[1])} bands, log-mel 0 has {int(mels[0].shape[1])}")
    n_mels = int(mels[0].shape[1])
    w = cepstrum_matrix(n_mels, n_coef, log_base)
    ctx = Context.get()
    xs = [ctx.to_device(m) for m in mels]
    x = xs[0] if len(xs) == 1 else torch.cat(xs)
    y = ctx.empty((int(x.shape[0]), w.shape[1]))
    _capi.check(ctx.lib.pk_op_matmul(ctx.handle, dptr(x), int(x.shape[0]), n_mels, int(w.shape[1]), _capi.fptr(w), None, dptr(y)))
    out = [wrap(t) for t in torch.split(y, [int(t.shape[0]) for t in xs])]
    return out[0] if single else out


def mcd_result(sum_sqrt, length, rows, cols):
    """MCD [dB] = (10 / ln 10) sqrt(2) sum_p sqrt(sum_k (c_k - c'_k)^2) / P, with the path's length P, the frame counts N, M
    and the length ratio M / N."""
    return dict(mcd=10.0 / math.log(10.0) * math.sqrt(2.0) * float(sum_sqrt) / int(length), length=int(length), rows=int(rows),
                cols=int(cols), length_ratio=int(cols) / int(rows))


def f0_result(sum_sq, n11, n10, n01, length):
    """log-F0 RMSE over the steps voiced in both tracks, sqrt(sum_sq / n11), in nats and in cents (x 1200 / ln 2); the V/UV
    error (n10 + n01) / P; n11.  No step voiced in both: the RMSE is NaN (no exception)."""
    rmse = math.sqrt(float(sum_sq) / int(n11)) if int(n11) > 0 else float("nan")
    return dict(f0_rmse=rmse, f0_rmse_cents=rmse * 1200.0 / math.log(2.0), vuv_error=(int(n10) + int(n01)) / int(length),
                voiced_both=int(n11))


def _listed(x, what):
    single = hasattr(x, "shape")
    xs = [x] if single else list(x)
    if not xs:
        raise ValueError(f"no {what} given")
    return xs, single


def mcd_batch(ref_logmels, syn_logmels, n_coef=13, log_base=10.0, *, return_paths=False):
    """Mel-cepstral distortion of synthesised against reference log-mels of different lengths: the DTW path over c_1 ...
    c_n_coef (c_0 excluded), then ``mcd_result`` per pair.  One pair or two lists.  ``return_paths``: also the ``DTWPath``s
    (for ``f0_batch``)."""
    refs, single = _listed(ref_logmels, "reference log-mels")
    syns, _ = _listed(syn_logmels, "synthesised log-mels")
    if len(refs) != len(syns):
        raise ValueError(f"{len(refs)} reference log-mels, {len(syns)} synthesised")
    if int(n_coef) < 1:
        raise ValueError(f"n_coef = {n_coef} must be at least 1")
    cr, cs = mel_cepstrum(list(refs), n_coef, log_base), mel_cepstrum(list(syns), n_coef, log_base)
    cols = (1, int(n_coef) + 1)
    paths = dtw_features(cr, cs, cols)
    stats = path_stats(paths, cr, cs, cols)
    out = [mcd_result(s.sum_sqrt, s.length, p.rows, p.cols) for s, p in zip(stats, paths)]
    if single:
        out, paths = out[0], paths[0]
    return (out, paths) if return_paths else out


def _log_f0(ctx, f0):
    """(frames,) Hz, 0 unvoiced -> ((frames, 1) float32 natural log, 0 where unvoiced; (frames,) uint8 voiced mask)."""
    t = ctx.to_device(f0).reshape(-1)
    voiced = t > 0
    return torch.where(voiced, torch.log(torch.where(voiced, t, torch.ones_like(t))), torch.zeros_like(t)).reshape(-1, 1), voiced


def f0_batch(paths, ref_f0, syn_f0):
    """log-F0 RMSE and V/UV error along given paths.  ``ref_f0`` / ``syn_f0``: f0 tracks in Hz on the frames the paths index
    (0: unvoiced), one pair or two lists.  Returns ``f0_result`` per pair."""
    refs, single = _listed(ref_f0, "reference f0 tracks")
    syns, _ = _listed(syn_f0, "synthesised f0 tracks")
    plist = [paths] if single and not isinstance(paths, (list, tuple)) else list(paths)
    if not (len(refs) == len(syns) == len(plist)):
        raise ValueError(f"{len(plist)} paths, {len(refs)} reference f0 tracks, {len(syns)} synthesised")
    ctx = Context.get()
    lr, ls = [_log_f0(ctx, f) for f in refs], [_log_f0(ctx, f) for f in syns]
    stats = path_stats(plist, [a for a, _ in lr], [a for a, _ in ls], None, [v for _, v in lr], [v for _, v in ls])
    out = [f0_result(s.sum_sq, s.n11, s.n10, s.n01, s.length) for s in stats]
    return out[0] if single else out


def score_batch(ref_wavs, syn_wavs, sr, mel=None, pitch=None, n_coef=13):
    """MCD, log-F0 RMSE and V/UV error of synthesised against recorded signals at rate ``sr`` (lists of 1-D arrays / tensors).
    ``mel``: an ``audio.LogMelFBank`` (default: the project's 80-band configuration at ``sr``); ``pitch``: an ``audio.Pitch``
    at the same hop (default: 80 ... 400 Hz).  Per signal the log-mel and f0 frame counts are cut to their minimum when they
    differ by one.  Returns per pair the union of ``mcd_result`` and ``f0_result``."""
    from . import audio
    refs, syns = list(ref_wavs), list(syn_wavs)
    if not refs or len(refs) != len(syns):
        raise ValueError(f"{len(refs)} reference signals, {len(syns)} synthesised")
    mel = audio.LogMelFBank(sr=sr) if mel is None else mel
    pitch = audio.Pitch(sr=sr, hop_length=mel.hop_length, f0min=80, f0max=400) if pitch is None else pitch
    if int(mel.sr) != int(sr) or int(pitch.sr) != int(sr) or int(mel.hop_length) != int(pitch.hop_length):
        raise ValueError(f"mel (sr {mel.sr}, hop {mel.hop_length}) and pitch (sr {pitch.sr}, hop {pitch.hop_length}) must share "
                         f"the rate {sr} and one hop")
    feats = []
    for wavs in (refs, syns):
        mels = mel.get_log_mel_fbank_batch(wavs)
        f0s = [f for f, _ in pitch.track(wavs)]
        for b, (m, f) in enumerate(zip(mels, f0s)):
            if abs(int(m.shape[0]) - int(f.shape[0])) > 1:
                raise ValueError(f"signal {b}: {int(m.shape[0])} log-mel frames, {int(f.shape[0])} f0 frames")
            n = min(int(m.shape[0]), int(f.shape[0]))
            mels[b], f0s[b] = m[:n], f[:n]
        feats.append((mels, f0s))
    mcd, paths = mcd_batch(feats[0][0], feats[1][0], n_coef, 10.0, return_paths=True)
    f0 = f0_batch(paths, feats[0][1], feats[1][1])
    return [dict(a, **b) for a, b in zip(mcd, f0)]
