"""The resampler's definition as an fp64 direct sum (a plain module, not a conftest).

    y[n] = sum_m x[m] g(n M / L - m),  n = 0 ... ceil(N L / M) - 1,  x = 0 outside 0 ... N - 1
    g(tau) = s rolloff sinc(rolloff s tau) K(s tau / zeros) for |s tau| < zeros, else 0;  s = min(1, L / M)
    K(u) = I0(beta sqrt(1 - u^2)) / I0(beta)

Nothing here calls parakeet_amd: the filter is written out again from the formula.  tau is kept as the integer
q = n M - m L over L, so that the support test |s tau| < zeros is decided exactly.
"""
import numpy as np

FILTERS = {
    "kaiser_best": (64, 0.9475937167399596, 14.769656459379492),
    "kaiser_fast": (16, 0.85, 8.555504641634386),
}


def g_of_q(q, L, M, zeros, rolloff, beta):
    """g(q / L) for an int64 array q."""
    q = np.asarray(q, dtype=np.int64)
    big = max(L, M)
    st = q.astype(np.float64) / big                       # s tau = (L / big) (q / L)
    inside = np.abs(q) < zeros * big
    u = np.where(inside, st / zeros, 0.0)
    s = min(1.0, L / M)
    val = s * rolloff * np.sinc(rolloff * st) * np.i0(beta * np.sqrt(1.0 - u * u)) / np.i0(beta)
    return np.where(inside, val, 0.0)


def out_len(N, L, M):
    return -(-N * L // M)


def _rows(x, L, M, zeros, rolloff, beta, n_lo, n_hi):
    """(weights, samples), both (n_hi - n_lo, width): every input sample that can reach an output, zero outside the signal."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    half = int(np.ceil(zeros * max(L, M) / L)) + 1
    n = np.arange(n_lo, n_hi, dtype=np.int64)
    base = n * M // L
    m = base[:, None] + np.arange(-half, half + 1, dtype=np.int64)[None, :]
    w = g_of_q(n[:, None] * M - m * L, L, M, zeros, rolloff, beta)
    ok = (m >= 0) & (m < N)
    return w, np.where(ok, x[np.clip(m, 0, N - 1)], 0.0)


def resample_ref(x, L, M, res_type="kaiser_best", n_lo=0, n_hi=None, with_abs=False, chunk=2048):
    """Outputs n_lo ... n_hi - 1 (default: all) in float64; with_abs: also sum_m |x[m]| |g|."""
    zeros, rolloff, beta = FILTERS[res_type] if isinstance(res_type, str) else res_type
    n_hi = out_len(len(x), L, M) if n_hi is None else n_hi
    y = np.empty(n_hi - n_lo)
    a = np.empty(n_hi - n_lo)
    for lo in range(n_lo, n_hi, chunk):
        hi = min(lo + chunk, n_hi)
        w, xs = _rows(x, L, M, zeros, rolloff, beta, lo, hi)
        y[lo - n_lo:hi - n_lo] = (w * xs).sum(axis=1)
        a[lo - n_lo:hi - n_lo] = (np.abs(w) * np.abs(xs)).sum(axis=1)
    return (y, a) if with_abs else y


def abs_dot(x, L, M, res_type="kaiser_best", n_lo=0, n_hi=None):
    """sum_m |x[m]| |g(n M / L - m)| per output: what the rounding bound of an fp32 evaluation scales with."""
    return resample_ref(x, L, M, res_type, n_lo, n_hi, with_abs=True)[1]
