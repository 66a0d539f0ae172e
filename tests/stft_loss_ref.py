"""fp64 restatement of parakeet/modules/stft_loss.py with a derived error bound for the engine's fp32 evaluation (a plain
module, not a conftest; shared by tests/test_stft_loss_cpu.py and tests/test_stft_loss_gpu.py).

Semantics, op order as in the reference: ``stft`` (:20-67) reflect-pads by n_fft/2, frames at stride hop, multiplies by the
window (scipy ``get_window(..., fftbins=True)`` centred in n_fft), transforms and returns ``sqrt(clip(re^2 + im^2, 1e-7))``;
``SpectralConvergenceLoss`` (:90-92) ``norm(y - x) / clip(norm(y), 1e-10)``; ``LogSTFTMagnitudeLoss`` (:116-118)
``mean |log(clip(y, eps)) - log(clip(x, eps))|``; ``MultiResolutionSTFTLoss`` (:205-219) the mean of both over the
resolutions.  The window is the float32 one the engine is handed and the two floors are the float32 values of 1e-7, as in a
float32 framework; everything else is float64.

The bound (``Field``, ``term_bounds``, ``sums_with_bound``, ``loss_bounds``).  Nothing in it comes from an observed error.
  re, im   fp32_bounds.dot_bound(|A| . |W|, n_fft): 2 (K + 2) u |A| . |W| with A the frame, W the windowed basis.
  p        = re^2 + im^2: fp32_bounds.power_bound (2 |re| b_re + b_re^2 + ... plus the roundings of the expression).
  X        = sqrt(a), a = max(p, floor): max is 1-Lipschitz, so the computed a' is within b_p of a and, like a, >= floor:
             a' >= max(a - b_p, floor).  With sqrt(a') - sqrt(a) = (a' - a) / (sqrt(a') + sqrt(a)) this gives
             b_X = b_p / (X + sqrt(max(X^2 - b_p, floor))) + 2u (X + that) for sqrtf with one spare ulp.  Far above the
             floor it tends to b_p / (2 X) = (|re| b_re + |im| b_im) / X (plus the second-order and rounding terms of
             power_bound); at the floor it stays finite.
  ln X     both the exact and the computed argument are >= m = max(sqrt(floor), eps), so by the mean value theorem
             b_L = b_X / max(X - b_X, m), plus 4u max(|ln X|, 1) for logf (2 ulp) with spare.
  terms    d = Y - X: b_d = b_X + b_Y + u (|d| + b_X + b_Y);  (Y - X)^2: 2 |d| b_d + b_d^2 + u (|d| + b_d)^2;
             Y^2: 2 Y b_Y + b_Y^2 + u (Y + b_Y)^2;  |ln Y - ln X|: b_LY + b_LX + u (|ln Y - ln X| + b_LY + b_LX).
  sums     sum of the term bounds + gamma * sum (term + its bound), gamma = (n_bin + 8) u: a frame's n_bin terms are added
             in fp32 in some order ((n_bin - 1) u for any order, Higham (4.4)); the frames are added in fp64 (negligible,
             part of the spare).
"""
import functools

import numpy as np
import scipy.signal

import fp32_bounds as fb

POWER_FLOOR = float(np.float32(1e-7))
LOG_FLOOR = float(np.float32(1e-7))
NORM_FLOOR = 1e-10


@functools.lru_cache(maxsize=None)
def window64(r, name="hann"):
    """The float32 window the engine is handed (centred in n_fft), as float64."""
    w = scipy.signal.get_window(name, r.win, fftbins=True)
    left = (r.n_fft - r.win) // 2
    w = np.pad(w, (left, r.n_fft - r.win - left))
    return w.astype(np.float32).astype(np.float64)


def frames(x, r, shift=0):
    """(T,) -> (F, n_fft) float64 frames of the reflect-padded signal; ``shift``: a mutant's frame start offset."""
    x = np.pad(np.asarray(x, np.float64), (r.n_fft // 2, r.n_fft // 2), mode="reflect")
    F = 1 + (len(x) - r.n_fft) // r.hop
    if shift:
        x = np.concatenate([x, np.zeros(shift)])
    return np.stack([x[f * r.hop + shift:f * r.hop + shift + r.n_fft] for f in range(F)])


def spectrum(x, r):
    """(T,) -> (F, n_bin) complex128."""
    return np.fft.rfft(frames(x, r) * window64(r), axis=1)


def floored(p, floor=POWER_FLOOR):
    return np.sqrt(np.maximum(p, floor))


def magnitude(x, r, floor=POWER_FLOOR):
    """(T,) -> (F, n_bin): stft() of one signal."""
    s = spectrum(x, r)
    return floored(s.real ** 2 + s.imag ** 2, floor)


def stft(x, r):
    """(B, T) -> (B, F, n_bin)."""
    return np.stack([magnitude(row, r) for row in np.asarray(x)])


def terms(X, Y, eps=LOG_FLOOR):
    """-> the three term fields (Y - X)^2, Y^2, |ln Y - ln X| of magnitudes of any shape."""
    return (Y - X) ** 2, Y ** 2, np.abs(np.log(np.maximum(Y, eps)) - np.log(np.maximum(X, eps)))


def sums(X, Y, eps=LOG_FLOOR):
    return np.array([t.sum() for t in terms(X, Y, eps)])


def spectral_convergence(x_mag, y_mag):
    return np.sqrt(((y_mag - x_mag) ** 2).sum()) / max(np.sqrt((y_mag ** 2).sum()), NORM_FLOOR)


def log_stft_magnitude(x_mag, y_mag, eps=LOG_FLOOR):
    return np.mean(np.abs(np.log(np.maximum(y_mag, eps)) - np.log(np.maximum(x_mag, eps))))


def stft_loss(x, y, r):
    """(B, T) each -> (sc_loss, mag_loss) of one resolution, batch-global."""
    xm, ym = stft(x, r), stft(y, r)
    return spectral_convergence(xm, ym), log_stft_magnitude(xm, ym)


def multi_resolution(x, y, resolutions):
    x, y = np.asarray(x), np.asarray(y)
    if x.ndim == 3:
        x, y = x.reshape(-1, x.shape[2]), y.reshape(-1, y.shape[2])
    per = np.array([stft_loss(x, y, r) for r in resolutions])
    return per[:, 0].mean(), per[:, 1].mean()


def losses_from_sums(s, entries):
    """(..., 3) sums, entry count -> (sc, mag)."""
    s = np.asarray(s, np.float64)
    return np.sqrt(s[..., 0]) / np.maximum(np.sqrt(s[..., 1]), NORM_FLOOR), s[..., 2] / entries


# ---------------------------------------------------------------------------------------------------------------- bound
@functools.lru_cache(maxsize=None)
def abs_basis(r):
    """|cos| w and |sin| w, each (n_fft, n_bin)."""
    N, nb = r.n_fft, 1 + r.n_fft // 2
    ang = 2.0 * np.pi * ((np.arange(N)[:, None] * np.arange(nb)[None, :]) % N) / N
    w = window64(r)[:, None]
    return np.abs(np.cos(ang)) * w, np.abs(np.sin(ang)) * w


class Field:
    """Magnitude of one signal at one resolution with its bounds: X, b_X, L = ln max(X, eps), b_L."""

    def __init__(self, x, r, eps=LOG_FLOOR, floor=POWER_FLOOR):
        A = frames(x, r)
        s = np.fft.rfft(A * window64(r), axis=1)
        ac, as_ = abs_basis(r)
        absA = np.abs(A)
        b_re, b_im = fb.dot_bound(absA @ ac, r.n_fft), fb.dot_bound(absA @ as_, r.n_fft)
        b_p = fb.power_bound(s.real, s.imag, b_re, b_im)
        self.X = floored(s.real ** 2 + s.imag ** 2, floor)
        b = b_p / (self.X + np.sqrt(np.maximum(self.X ** 2 - b_p, floor)))
        self.b_X = b + 2.0 * fb.U * (self.X + b)
        m = max(np.sqrt(floor), eps)
        self.L = np.log(np.maximum(self.X, eps))
        self.b_L = self.b_X / np.maximum(self.X - self.b_X, m) + 4.0 * fb.U * np.maximum(np.abs(self.L), 1.0)


def term_bounds(fx, fy):
    """Bounds of the three term fields for two ``Field``s."""
    U = fb.U
    d = np.abs(fy.X - fx.X)
    b_d = fx.b_X + fy.b_X + U * (d + fx.b_X + fy.b_X)
    b0 = 2.0 * d * b_d + b_d ** 2 + U * (d + b_d) ** 2
    b1 = 2.0 * fy.X * fy.b_X + fy.b_X ** 2 + U * (fy.X + fy.b_X) ** 2
    dl = np.abs(fy.L - fx.L)
    b2 = fx.b_L + fy.b_L + U * (dl + fx.b_L + fy.b_L)
    return b0, b1, b2


def sums_with_bound(x, y, r, eps=LOG_FLOOR):
    """One pair -> (sums (3,), bound (3,), Field x, Field y)."""
    fx, fy = Field(x, r, eps), Field(y, r, eps)
    t = terms(fx.X, fy.X, eps)
    b = term_bounds(fx, fy)
    gamma = (fx.X.shape[1] + 8) * fb.U
    s = np.array([v.sum() for v in t])
    bs = np.array([bv.sum() + gamma * (v.sum() + bv.sum()) for v, bv in zip(t, b)])
    return s, bs, fx, fy


def loss_bounds(s, bs, entries):
    """Sums (3,) over a set of entries with their bounds -> (sc, mag, b_sc, b_mag): the quotient is monotone in both sums,
    so its bound is the larger distance to the two corners of the box."""
    sc, mag = losses_from_sums(s, entries)
    den_lo = max(np.sqrt(max(s[1] - bs[1], 0.0)), NORM_FLOOR)
    den_hi = max(np.sqrt(s[1] + bs[1]), NORM_FLOOR)
    hi = np.sqrt(s[0] + bs[0]) / den_lo
    lo = np.sqrt(max(s[0] - bs[0], 0.0)) / den_hi
    return sc, mag, max(hi - sc, sc - lo), bs[2] / entries


# ------------------------------------------------------------------------------------------- float32 path and mutants
def dense_f32(x, r, shift=0, drop_last=False, floor=POWER_FLOOR):
    """The dense-DFT path in float32 numpy: frames @ windowed basis, magnitude, all in float32.  -> (F, n_bin) float32."""
    N, nb = r.n_fft, 1 + r.n_fft // 2
    ang = -2.0 * np.pi * ((np.arange(N)[:, None] * np.arange(nb)[None, :]) % N) / N
    w = window64(r)[:, None]
    Wc, Ws = (np.cos(ang) * w).astype(np.float32), (np.sin(ang) * w).astype(np.float32)
    A = frames(x, r, shift).astype(np.float32)
    if drop_last:
        A = A[:-1]
    re, im = A @ Wc, A @ Ws
    return np.sqrt(np.maximum(re * re + im * im, np.float32(floor)))


def sums_f32(X, Y, eps=LOG_FLOOR):
    """The three sums the way the kernels form them: terms and a frame's sum in float32, frames in float64."""
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    e = np.float32(eps)
    d = Y - X
    t = (d * d, Y * Y, np.abs(np.log(np.maximum(Y, e)) - np.log(np.maximum(X, e))))
    return np.array([v.sum(axis=1, dtype=np.float32).astype(np.float64).sum() for v in t])


def mutants(x, y, r, silent_x=False):
    """{name: (sums (3,), (X, Y) magnitudes or None)} of subtly wrong evaluations of one pair; the magnitudes are given
    where they keep their shape, so that they can be held against the per-entry bound as well.  ``floor`` is returned for a
    silent x only."""
    X, Y = magnitude(x, r), magnitude(y, r)
    late = [floored(np.abs(np.fft.rfft(frames(v, r, 1) * window64(r), axis=1)) ** 2) for v in (x, y)]
    out = {
        "last_frame": (sums(X[:-1], Y[:-1]), None),
        "nyquist": (sums(X[:, :-1], Y[:, :-1]), None),
        "off_by_one": (sums(*late), tuple(late)),
    }
    if silent_x:
        Xf = magnitude(x, r, 1e-10)
        out["floor"] = (sums(Xf, Y), (Xf, Y))
    return out
