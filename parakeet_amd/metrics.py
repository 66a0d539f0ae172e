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
data and forms the logarithm / voicing mask of the f0 tracks.

Intelligibility of time-aligned pairs: ``stoi_batch`` / ``stoi`` give STOI (Taal et al. 2011) and ESTOI (Jensen
& Taal 2016) of a degraded signal against the clean one, as this project restates the papers (csrc/pk_stoi.h; NOT pystoi, NOT
the MATLAB code: the resampler in front is ``audio.Resample``, fewer than 30 spectrum frames give NaN with 0 segments, and nobody
has compared the numbers with another toolkit's on speech).  Every stage runs on the engine; the host reads the results once.

Programme loudness: ``loudness_batch`` / ``loudness`` give the gated loudness of ITU-R BS.1770-4 in LUFS for
mono signals, as this project restates the Recommendation (csrc/pk_iir.h; NOT pyloudnorm, NOT libebur128: blocks lie on a
100 ms sample grid, which needs ``sr % 10 == 0``, and nobody has compared the numbers with another meter's on speech)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi
from .alignment import dtw_features, path_stats
from .runtime import Context, dptr, wrap

__all__ = ["dct_matrix", "mel_cepstrum", "mcd_result", "f0_result", "mcd_batch", "f0_batch", "score_batch",
           "stoi", "stoi_batch", "stoi_silent_frames", "stoi_bands", "stoi_from_bands", "stoi_num_frames", "stoi_band_edges",
           "loudness", "loudness_batch"]

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


# ------------------------------------------------------------------------------------- STOI / ESTOI (4.7d)
STOI_FS, STOI_BANDS, STOI_SEGMENT = 10000, 15, 30
_STOI_RESULT = np.dtype([("d", "<f8"), ("segments", "<i4"), ("kept", "<i4"), ("frames", "<i4"), ("reserved", "<i4")])


def stoi_num_frames(n_samples):
    """F(L): frames of 256 samples at hop 128 that start strictly below L - 256 (``pk_stoi_num_frames``)."""
    out = C.c_int64()
    _capi.check(_capi.lib().pk_stoi_num_frames(int(n_samples), C.byref(out)))
    return out.value


def stoi_band_edges():
    """(lo, hi): int32 arrays of the 15 one-third-octave bands' bins [lo, hi) of the 512-point transform at 10 kHz."""
    lo, hi = np.zeros(STOI_BANDS, np.int32), np.zeros(STOI_BANDS, np.int32)
    _capi.check(_capi.lib().pk_stoi_band_edges(lo.ctypes.data_as(C.POINTER(C.c_int32)), hi.ctypes.data_as(C.POINTER(C.c_int32))))
    return lo, hi


def _stoi_signals(wavs, what):
    """A list of 1-D signals -> (list of 1-D host / device arrays, lengths); nothing touches the device yet."""
    xs, single = _listed(wavs, what)
    for b, x in enumerate(xs):
        if not hasattr(x, "shape") or len(x.shape) != 1:
            raise ValueError(f"{what} {b}: expected a 1-D signal, got " + (f"shape {tuple(x.shape)}" if hasattr(x, "shape")
                                                                          else type(x).__name__))
    return xs, single


def _stoi_pack(ctx, xs):
    ts = [ctx.to_device(x).reshape(-1) for x in xs]
    offs = np.zeros(len(ts) + 1, np.int64)
    offs[1:] = np.cumsum([t.numel() for t in ts])
    x = ts[0] if len(ts) == 1 else torch.cat(ts)
    if x.numel() == 0:
        x = ctx.empty((1,))                                 # a pointer to pass; nothing of it is read
    return x, offs


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def stoi_silent_frames(ref_wavs):
    """Stage 1 alone (``pk_stoi_mask``): clean signals at 10 kHz -> per signal ``(keep, energy)``: a bool array over its F(L)
    frames (kept iff within 40 dB of the loudest) and the frame energies in dB, float32."""
    xs, single = _stoi_signals(ref_wavs, "signal")
    ctx = Context.get()
    x, offs = _stoi_pack(ctx, xs)
    nf = [stoi_num_frames(int(offs[b + 1] - offs[b])) for b in range(len(xs))]
    tot = max(sum(nf), 1)
    e, keep, kept = ctx.empty((tot,)), ctx.empty((tot,), dtype=torch.uint8), ctx.empty((len(xs),), dtype=torch.int32)
    _capi.check(ctx.lib.pk_stoi_mask(ctx.handle, dptr(x), _i64p(offs), len(xs), dptr(e), dptr(keep), None, dptr(kept)))
    e, keep, kept = e.cpu().numpy(), keep.cpu().numpy().astype(bool), kept.cpu().numpy()
    out, o = [], 0
    for b, n in enumerate(nf):
        assert int(keep[o:o + n].sum()) == int(kept[b])
        out.append((keep[o:o + n], e[o:o + n]))
        o += n
    return out[0] if single else out


def stoi_bands(wavs):
    """Stage 3 alone (``pk_stoi_bands``): signals at 10 kHz -> per signal a device tensor (F(L), 15) of one-third-octave band
    magnitudes of its frames (Hann window of 256, zero-padded to 512, the radix FFT)."""
    xs, single = _stoi_signals(wavs, "signal")
    ctx = Context.get()
    x, offs = _stoi_pack(ctx, xs)
    nf = [stoi_num_frames(int(offs[b + 1] - offs[b])) for b in range(len(xs))]
    out = ctx.empty((max(sum(nf), 1), STOI_BANDS))
    _capi.check(ctx.lib.pk_stoi_bands(ctx.handle, dptr(x), _i64p(offs), len(xs), dptr(out)))
    res = [wrap(t) for t in torch.split(out[:sum(nf)], nf)]
    return res[0] if single else res


def stoi_from_bands(ref_bands, deg_bands, extended=False):
    """Stage 4 alone (``pk_stoi_segments``): (frames, 15) band magnitudes of clean and degraded signals -> per pair
    ``(d, segments)``; fewer than 30 frames: (nan, 0)."""
    xs, single = _listed(ref_bands, "reference bands")
    ys, _ = _listed(deg_bands, "degraded bands")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} reference band matrices, {len(ys)} degraded")
    for b, (x, y) in enumerate(zip(xs, ys)):
        if len(x.shape) != 2 or int(x.shape[1]) != STOI_BANDS or tuple(x.shape) != tuple(y.shape):
            raise ValueError(f"pair {b}: expected two (frames, {STOI_BANDS}) matrices of one shape, got {tuple(x.shape)} and "
                             f"{tuple(y.shape)}")
    ctx = Context.get()
    tx, ty = [ctx.to_device(x) for x in xs], [ctx.to_device(y) for y in ys]
    nf = np.array([int(t.shape[0]) for t in tx], np.int32)
    px, py = torch.cat(tx), torch.cat(ty)
    if px.numel() == 0:
        px = py = ctx.empty((1, STOI_BANDS))
    d, seg = ctx.empty((len(xs),), dtype=torch.float64), ctx.empty((len(xs),), dtype=torch.int32)
    _capi.check(ctx.lib.pk_stoi_segments(ctx.handle, dptr(px), dptr(py), nf.ctypes.data_as(C.POINTER(C.c_int32)), len(xs),
                                         1 if extended else 0, dptr(d), dptr(seg)))
    d, seg = d.cpu().numpy(), seg.cpu().numpy()
    out = [(float(a), int(s)) for a, s in zip(d, seg)]
    return out[0] if single else out


def stoi_batch(ref_wavs, deg_wavs, sr, extended=False, return_details=False):
    """STOI (``extended``: ESTOI) of degraded against clean signals at rate ``sr``: one pair or two lists of 1-D signals, each
    pair of one length (``ValueError`` otherwise: the measure is defined for time-aligned signals).  ``sr != 10000``: both are
    resampled to 10 kHz by ``audio.Resample(sr, 10000)`` on the engine.  Returns a float per pair, NaN where fewer than 30
    spectrum frames remain after silent-frame removal; ``return_details``: dicts with ``d``, ``segments``, ``kept_frames``
    (frames of the clean signal within 40 dB of its loudest) and ``frames``.  A ragged batch is one engine call; a pair's result
    is the same bits alone, in any batch and at any position."""
    xs, single = _stoi_signals(ref_wavs, "reference signal")
    ys, _ = _stoi_signals(deg_wavs, "degraded signal")
    if len(xs) != len(ys):
        raise ValueError(f"{len(xs)} reference signals, {len(ys)} degraded")
    for b, (x, y) in enumerate(zip(xs, ys)):
        if int(x.shape[0]) != int(y.shape[0]):
            raise ValueError(f"pair {b}: the reference has {int(x.shape[0])} samples, the degraded signal {int(y.shape[0])}; "
                             "STOI compares time-aligned signals of one length")
    if int(sr) != sr or int(sr) < 1:
        raise ValueError(f"sr = {sr} must be a positive integer")
    ctx = Context.get()
    if int(sr) != STOI_FS:
        from . import audio
        rs = audio._resampler(int(sr), STOI_FS)
        xs, ys = rs.run_batch(xs), rs.run_batch(ys)
    x, offs = _stoi_pack(ctx, xs)
    y, _ = _stoi_pack(ctx, ys)
    B = len(xs)
    res = torch.empty((B * _STOI_RESULT.itemsize,), dtype=torch.uint8, device=ctx.device)
    _capi.check(ctx.lib.pk_stoi_run(ctx.handle, dptr(x), dptr(y), _i64p(offs), B, 1 if extended else 0, dptr(res)))
    rec = res.cpu().numpy().view(_STOI_RESULT)               # the one read
    if return_details:
        out = [dict(d=float(r["d"]), segments=int(r["segments"]), kept_frames=int(r["kept"]), frames=int(r["frames"])) for r in rec]
    else:
        out = [float(r["d"]) for r in rec]
    return out[0] if single else out


def stoi(ref_wav, deg_wav, sr, extended=False):
    """``stoi_batch`` of one pair: a float."""
    if not hasattr(ref_wav, "shape") or not hasattr(deg_wav, "shape"):
        raise ValueError("stoi takes one pair of 1-D signals; lists go to stoi_batch")
    return stoi_batch(ref_wav, deg_wav, sr, extended)


# ------------------------------------------------------------------------------------- gated loudness (4.5h)
def loudness_batch(wavs, sr, return_details=False):
    """Gated programme loudness (ITU-R BS.1770-4, one channel of weight 1) of one signal or a list of 1-D float32 signals at
    rate ``sr``, in LUFS: K-weighting in float64, 400 ms blocks every 100 ms, the absolute gate at -70 LUFS and the relative
    gate 10 LU below the mean of what the first keeps; -inf where no block survives (a signal shorter than 400 ms, or silence).
    ``sr`` must be a multiple of 10 in 8 000 ... 192 000 (``NotImplementedError`` otherwise; resample first).  A float64 array
    per list, a float for one signal; ``return_details``: dicts with ``lufs``, ``blocks``, ``gated_abs``, ``gated``,
    ``mean_power``, ``relative_threshold_lufs`` and ``peak`` (the sample peak).  A ragged batch is one engine call with one read;
    an utterance's result is the same bits alone, in any batch and at any position."""
    from . import audio
    xs, single = _listed(wavs, "signal")
    _, _, _, m = audio._loudness_run(xs, sr)
    if not return_details:
        return float(m["lufs"][0]) if single else m["lufs"]
    out = []
    for b in range(len(xs)):
        rel = float(m["rel"][b])
        out.append(dict(lufs=float(m["lufs"][b]), blocks=int(m["blocks"][b]), gated_abs=int(m["gated_abs"][b]),
                        gated=int(m["gated"][b]), mean_power=float(m["mean_power"][b]),
                        relative_threshold_lufs=float(-0.691 + 10.0 * np.log10(rel)) if rel > 0 else -math.inf,
                        relative_threshold_power=rel, peak=float(m["peak"][b])))
    return out[0] if single else out


def loudness(wav, sr):
    """``loudness_batch`` of one signal: a float."""
    if not hasattr(wav, "shape"):
        raise ValueError("loudness takes one 1-D signal; lists go to loudness_batch")
    return loudness_batch(wav, sr)
