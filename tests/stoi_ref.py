"""STOI / ESTOI as csrc/pk_stoi.h defines them, restated in float64 numpy; an fp32 evaluation of the engine's plan; the bounds
the GPU tests use, with their derivations (a plain module, not a conftest; shared by tests/test_stoi_cpu.py and
tests/test_stoi_gpu.py).  This is the project's own restatement of Taal et al. 2011 and Jensen & Taal 2016, NOT pystoi.

THE DEFINITION.  fs = 10 kHz, frames of 256 at hop 128, w = numpy.hanning(258)[1:-1], FFT 512, J = 15 one-third-octave bands from
150 Hz, N = 30 frames per segment, beta = -15 dB, dynamic range 40 dB, EPS = 2^-52.
  frames    start at 0, 128, ... strictly below L - 256: F(L) = 0 for L <= 256, else (L - 257) // 128 + 1.
  1 mask    e_i = 20 log10(||w x_i|| + EPS) on the clean signal; frame i is kept iff max e - 40 - e_i < 0; both signals are
            rebuilt from their windowed kept frames by overlap-add at hop 128: K kept frames give (K - 1) 128 + 256 samples
            and K - 1 spectrum frames.
  2 bands   every frame of a rebuilt signal times w, zero-padded to 512, rfft; band j = sqrt(sum_{lo_j <= k < hi_j} |X_k|^2).
  3 segments  m = 0 ... S - 1, S = (K - 1) - 29: the 15 x 30 blocks x, y of frames [m, m + 30).
            STOI per band row: a = ||x|| / (||y|| + EPS); y' = min(a y, x (1 + 10^(15/20))); rows minus their means, divided
            by (norm + EPS); d = sum xh yh' / (J S).
            ESTOI: rows normalised like that (no clipping), then columns the same way; d = sum xh yh / (N S).
  S <= 0: d = NaN, segments = 0 (documented; not pystoi's 1e-5).

THE BOUNDS.  u = 2^-24 (fp32_bounds.U), eps = 2^-53.

bands (``band_bound``).  The engine transforms the float32 frame with the plan of csrc/pk_rfft.h; tests/rfft_ref.py derives
|dX_k| <= RFFT_C(512) u S for every bin, S = sum_n |x_n w_n| of the frame (its window budget of two roundings covers a window
prepared in float64 and rounded, and the product).  A band is the 2-norm of nb = hi - lo bins: the exact norm of the perturbed
bins differs from the true one by at most ||dX||_2 <= sqrt(nb) RFFT_C u S (triangle inequality).  The engine then forms
s = sum (re re + im im) in float32: two products and one addition per bin (each term carries (1 + u)^2), nb - 1 further
additions of non-negative terms: a relative error of at most gamma(nb + 1) = (nb + 1) u / (1 - (nb + 1) u) on s, half of it
(to first order; the whole of it is taken here) on sqrt(s), and u for the correctly rounded square root:
    |d band| <= sqrt(nb) RFFT_C(512) u S + (gamma(nb + 1) + u) (band + sqrt(nb) RFFT_C(512) u S).

segments (``stoi_seg_bound`` / ``estoi_seg_bound``).  Engine and numpy evaluate the same float64 formulas on the same float32
bands in different summation orders; every operation rounds with relative error eps, the double ``sqrt`` of HIP's math API
table is listed with 1 ulp = 2 eps (as tests/test_dtw_gpu.py cites it).  First-order count, in units of eps, for a row v of
30 non-negative values whose entries carry a relative error e_in, with kappa >= ||v|| / ||v - mean||:
  * ||v||: 30 squares and 29 additions are 30 on the sum of squares, 15 on its root, 2 for the root: 17.
  * a = ||x|| / (||y|| + EPS): 17 + 17 + 1 + 1 = 36; a y_n: 37; x_n c: 1 (c is the same constant on both sides); the minimum
    moves by at most the larger error of its arguments (whichever branch either side takes): e_in = 37 for y', 0 for x and for
    ESTOI's y.
  * mean = (sum v) / 30: (29 + e_in) sum|v| and the division: |d mean| <= (30 + e_in) sum|v| / 30 <= (30 + e_in) ||v|| / sqrt(30).
  * c = v - mean: ||dc|| <= e_in ||v|| + sqrt(30) |d mean| + ||c|| <= ((30 + 2 e_in) kappa + 1) ||c|| =: E_c ||c||.
  * ||c|| + EPS: E_c + 17 + 1; h = c / that: ||dh|| <= 2 E_c + 19 (||h|| <= 1).
  * a row's sum_n xh_n yh_n: the two vectors' errors plus 30 for the products and additions (sum |xh yh| <= 1):
    2 E_cx + 2 E_cy + 68.
  STOI: E_cx = 30 kappa + 1, E_cy = 104 kappa + 1: a row's value moves by at most (268 kappa + 72) eps.  d is the mean of J S
  such values: the same bound, plus the additions over rows and segments (14 + ceil(S / 256) + 8 on |d| <= 1) and the division.
  ESTOI: a row-normalised value carries an ABSOLUTE error of at most E_r = 2 (30 kappa + 1) + 19 = 60 kappa + 21 (entries of a
  unit vector).  A column g of 15 such values: |d mean| <= E_r + 15 ||g|| / sqrt(15); ||dc|| <= 2 sqrt(15) E_r + 15 ||g|| + ||c||,
  that is E_col = 2 sqrt(15) E_r / cmin + 15 kappa + 1 relative to ||c|| >= cmin, the smallest centred column norm of the
  inputs (the tests assert cmin >= 0.05 on theirs); ||c|| + EPS: E_col + 10 + 1; the normalised column: 2 E_col + 12; a column's
  sum_j xh yh: 2 E_colx + 2 E_coly + 24 + 15.  d is the mean of N S such values, plus 29 + ceil(S / 256) + 8 + 1.
  Each side carries such an error; the bound on their difference is twice it, and once more doubled for the second-order terms.
"""
import numpy as np

import fp32_bounds as fb
import rfft_ref as rr

FS, FRAME, HOP, NFFT, J, N = 10000, 256, 128, 512, 15, 30
BETA_DB, RANGE_DB = -15.0, 40.0
EPS = 2.0 ** -52
CLIP = 1.0 + 10.0 ** (-BETA_DB / 20.0)
WINDOW = np.hanning(FRAME + 2)[1:-1]
WINDOW32 = WINDOW.astype(np.float32)
WINDOW512 = np.concatenate([WINDOW32, np.zeros(NFFT - FRAME, np.float32)])
SQRT_ULP = 1                      # HIP math API table: sqrt (double), maximum ulp error (tests/test_dtw_gpu.py)
E64 = 2.0 ** -53


def num_frames(L):
    return 0 if L <= FRAME else (L - FRAME - 1) // HOP + 1


def band_edges():
    """(lo, hi): band j sums the bins [lo[j], hi[j]); the bins nearest to 150 * 2^((2 j -+ 1) / 6) Hz on the grid k fs / 512."""
    f = np.arange(NFFT // 2 + 1, dtype=np.float64) * FS / NFFT
    j = np.arange(J, dtype=np.float64)
    fl, fh = 150.0 * 2.0 ** ((2 * j - 1) / 6.0), 150.0 * 2.0 ** ((2 * j + 1) / 6.0)
    lo = np.array([int(np.argmin((f - a) ** 2)) for a in fl])
    hi = np.array([int(np.argmin((f - a) ** 2)) for a in fh])
    return lo, hi


def _frames(x, dtype):
    """(F(L), 256): the frames of x (not windowed)."""
    x = np.asarray(x, dtype)
    F = num_frames(len(x))
    if F == 0:
        return np.zeros((0, FRAME), dtype)
    idx = np.arange(F)[:, None] * HOP + np.arange(FRAME)[None, :]
    return x[idx]


def _overlap_add(fr, dtype):
    """windowed frames (K, 256) -> (K - 1) 128 + 256 samples (none for K = 0), the earlier frame added first"""
    K = fr.shape[0]
    if K == 0:
        return np.zeros(0, dtype)
    out = np.zeros((K + 1) * HOP, dtype)
    for k in range(K):
        out[k * HOP:k * HOP + FRAME] = out[k * HOP:k * HOP + FRAME] + fr[k]
    return out


def silent_mask(x):
    """clean signal -> (keep (F,) bool, e (F,) float64 dB)"""
    fr = _frames(x, np.float64) * WINDOW
    e = 20.0 * np.log10(np.sqrt(np.sum(fr * fr, axis=1)) + EPS)
    if len(e) == 0:
        return np.zeros(0, bool), e
    return (np.max(e) - RANGE_DB - e) < 0, e


def threshold_margin(x):
    """min over frames of |max e - 40 - e_i| in dB (inf without frames): the tests' condition on their inputs"""
    _, e = silent_mask(x)
    return float(np.min(np.abs(np.max(e) - RANGE_DB - e))) if len(e) else np.inf


def rebuild(x, keep):
    return _overlap_add((_frames(x, np.float64) * WINDOW)[keep], np.float64)


def bands(x):
    """signal -> (F(L), 15) float64 band magnitudes of its frames"""
    fr = _frames(x, np.float64) * WINDOW
    X = np.fft.rfft(fr, n=NFFT, axis=1)
    P = X.real ** 2 + X.imag ** 2
    lo, hi = band_edges()
    return np.stack([np.sqrt(P[:, a:b].sum(axis=1)) for a, b in zip(lo, hi)], axis=1).reshape(-1, J)


def _blocks(b):
    """(frames, 15) -> (S, 15, 30): segment m holds frames [m, m + 30)"""
    S = b.shape[0] - (N - 1)
    idx = np.arange(S)[:, None] + np.arange(N)[None, :]
    return np.transpose(np.asarray(b, np.float64)[idx], (0, 2, 1))


def _norm_last(v):
    v = v - v.mean(axis=-1, keepdims=True)
    return v / (np.sqrt(np.sum(v * v, axis=-1, keepdims=True)) + EPS)


def segments(xb, yb, extended=False, details=False):
    """(frames, 15) band magnitudes of clean and degraded -> (d, S); fewer than 30 frames: (nan, 0).  ``details``: also the
    conditioning of the inputs: dict(kappa: the largest ||v|| / ||v - mean|| over the rows (and ESTOI's columns), cmin: the
    smallest centred column norm)."""
    S = xb.shape[0] - (N - 1)
    if S <= 0:
        return (float("nan"), 0, dict(kappa=0.0, cmin=np.inf)) if details else (float("nan"), 0)
    x, y = _blocks(xb), _blocks(yb)

    def kap(v, axis):
        c = v - v.mean(axis=axis, keepdims=True)
        nv, nc = np.sqrt((v * v).sum(axis)), np.sqrt((c * c).sum(axis))
        return (float(np.max(nv / nc)) if np.all(nc > 0) else np.inf), float(np.min(nc))

    info = dict(kappa=max(kap(x, -1)[0], kap(y, -1)[0]), cmin=np.inf)
    if not extended:
        a = np.sqrt(np.sum(x * x, axis=-1, keepdims=True)) / (np.sqrt(np.sum(y * y, axis=-1, keepdims=True)) + EPS)
        yp = np.minimum(a * y, x * CLIP)
        info["kappa"] = max(info["kappa"], kap(yp, -1)[0])
        d = float(np.sum(_norm_last(x) * _norm_last(yp)) / (J * S))
    else:
        xr, yr = _norm_last(x), _norm_last(y)
        (kx, cx), (ky, cy) = kap(xr, 1), kap(yr, 1)
        info["kappa"], info["cmin"] = max(info["kappa"], kx, ky), min(cx, cy)
        xc = np.swapaxes(_norm_last(np.swapaxes(xr, 1, 2)), 1, 2)
        yc = np.swapaxes(_norm_last(np.swapaxes(yr, 1, 2)), 1, 2)
        d = float(np.sum(xc * yc) / (N * S))
    return (d, S, info) if details else (d, S)


def stoi(x, y, extended=False):
    """clean, degraded at 10 kHz, one length -> dict(d, segments, kept, frames), float64 throughout"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.shape == y.shape and x.ndim == 1
    keep, _ = silent_mask(x)
    d, S = segments(bands(rebuild(x, keep)), bands(rebuild(y, keep)), extended)
    return dict(d=d, segments=S, kept=int(keep.sum()), frames=len(keep))


# ------------------------------------------------------------------------------------- the engine's plan in float32 numpy
def frame_power_f32(x):
    """ss (F,) float32 of the clean signal in the order of csrc/pk_stoi.h: lane l adds n = l, l + 64, l + 128, l + 192, then the
    butterfly over lanes (numpy has no fused multiply-add: the product p p is rounded once more than on the device)."""
    p = _frames(x, np.float32) * WINDOW32
    F = p.shape[0]
    acc = np.zeros((F, 64), np.float32)
    for q in range(FRAME // 64):
        acc = p[:, 64 * q:64 * q + 64] * p[:, 64 * q:64 * q + 64] + acc
    lanes = np.arange(64)
    for h in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ h]
    assert acc.dtype == np.float32
    return acc[:, 0]


def silent_mask_f32(x):
    ss = frame_power_f32(x)
    if len(ss) == 0:
        return np.zeros(0, bool)
    e = 20.0 * np.log10(np.sqrt(ss.astype(np.float64)) + EPS)
    return (np.max(e) - RANGE_DB - e) < 0


def rebuild_f32(x, keep):
    return _overlap_add((_frames(x, np.float32) * WINDOW32)[keep], np.float32)


def bands_f32(x):
    """float32 signal -> (F(L), 15) float32: rfft_ref's plan at n = 512 on the zero-padded signal with the window w | zeros,
    power and range sums in float32 ascending, float32 square root"""
    x = np.asarray(x, np.float32)
    F = num_frames(len(x))
    if F == 0:
        return np.zeros((0, J), np.float32)
    xp = np.concatenate([x, np.zeros(NFFT, np.float32)])
    rows = xp[np.arange(F)[:, None] * HOP + np.arange(NFFT)[None, :]]
    spec = rr.rfft_f32(rows, window=WINDOW512)
    re, im = spec[:, :NFFT // 2 + 1], spec[:, NFFT // 2 + 1:]
    P = re * re + im * im
    lo, hi = band_edges()
    out = np.zeros((F, J), np.float32)
    for j, (a, b) in enumerate(zip(lo, hi)):
        s = np.zeros(F, np.float32)
        for k in range(a, b):
            s = s + P[:, k]
        out[:, j] = np.sqrt(s)
    assert out.dtype == np.float32
    return out


def stoi_f32(x, y, extended=False):
    """The engine's plan: float32 up to the bands, float64 segments."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    keep = silent_mask_f32(x)
    d, S = segments(bands_f32(rebuild_f32(x, keep)), bands_f32(rebuild_f32(y, keep)), extended)
    return dict(d=d, segments=S, kept=int(keep.sum()), frames=len(keep))


# ------------------------------------------------------------------------------------- the bounds (module docstring)
def band_bound(x, want):
    """float32 signal x, want = bands(x) (F, 15) -> (F, 15): the bound on |engine band - want|"""
    fr = np.abs(_frames(x, np.float64) * WINDOW)
    S = fr.sum(axis=1, keepdims=True)
    lo, hi = band_edges()
    nb = (hi - lo).astype(np.float64)[None, :]
    spec_err = np.sqrt(nb) * rr.rfft_c(NFFT) * fb.U * S
    gamma = (nb + 1) * fb.U / (1.0 - (nb + 1) * fb.U)
    return spec_err + (gamma + fb.U) * (np.asarray(want, np.float64) + spec_err)


def _tree(S):
    return -(-max(S, 1) // 256) + 8


def stoi_seg_bound(kappa, S):
    one = 268.0 * kappa + 72.0 + (14 + _tree(S)) + 1
    return 4.0 * one * E64


def estoi_seg_bound(kappa, cmin, S):
    e_r = 60.0 * kappa + 21.0
    e_col = 2.0 * np.sqrt(15.0) * e_r / cmin + 15.0 * kappa + 1.0
    one = 4.0 * e_col + 39.0 + (29 + _tree(S)) + 1
    return 4.0 * one * E64


# ------------------------------------------------------------------------------------- test signals
def harmonic(L, seed, f0=140.0):
    """A harmonic test signal of L samples at 10 kHz: eight partials of a gliding fundamental under a slow envelope, float32"""
    r = np.random.default_rng([L, seed])
    t = np.arange(L) / FS
    f = f0 * (1.0 + 0.15 * np.sin(2 * np.pi * 1.3 * t + r.uniform(0, 6)))
    ph = 2 * np.pi * np.cumsum(f) / FS
    amp = r.uniform(0.2, 1.0, 8) / np.arange(1, 9)
    x = sum(a * np.sin(k * ph + r.uniform(0, 6)) for k, a in zip(range(1, 9), amp))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + r.uniform(0, 6))
    return (0.3 * env * x + 1e-3 * r.normal(size=L)).astype(np.float32)


def add_noise(x, snr_db, seed):
    r = np.random.default_rng([len(x), seed, 7])
    n = r.normal(size=len(x))
    n *= np.sqrt(np.sum(np.asarray(x, np.float64) ** 2) / np.sum(n * n)) * 10.0 ** (-snr_db / 20.0)
    return (np.asarray(x, np.float64) + n).astype(np.float32)
