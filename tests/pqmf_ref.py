"""fp64 restatement of the pseudo-QMF bank of csrc/pk_pqmf.h with derived bounds for the engine's fp32 evaluation (a plain
module, not a conftest; shared by tests/test_pqmf_cpu.py and tests/test_pqmf_gpu.py).

Filters (float64, rounded once to float32; K = subbands, n = 0 ... taps, c = n - taps / 2):
  proto[n]       = sin(pi cutoff c) / (pi c) * kaiser(taps + 1, beta)[n], the centre tap is cutoff
  analysis_k[n]  = 2 proto[n] cos((2 k + 1) pi / (2 K) c + (-1)^k pi / 4);   synthesis_k[n]: the same with - (-1)^k pi / 4
``cutoff`` and ``beta`` are the float32 values the C ABI carries.  The Kaiser window is I0 by its power series, as in the header.

Operations (h = taps / 2):
  analysis   bands[k, m] = sum_(n = 0 ... taps) analysis_k[n] x[m K + n - h], x = 0 outside [0, L); M = floor(L / K)
  synthesis  wav[t] = K sum_k sum_m synthesis_k[m K - t + h] bands[k, m] over the m with 0 <= m K - t + h <= taps

Bounds.  The engine contracts every product into one fmaf: one rounding per term, so Higham's dot-product bound
(fp32_bounds.dot_bound, which allows a rounding for the product AND one for the sum) holds with room.  K is the number of
products an output really sums: taps + 1 for analysis (the kernel multiplies the staged zeros outside the utterance too;
they add exactly 0), subbands * ceil((taps + 1) / subbands) at most for synthesis.  dot_bound's two spare roundings cover the
final product with (float)K of synthesis (exact for a power of two).  The filters are the engine's own float32 values
(pk_pqmf_filters): their rounding is not part of the arithmetic under test; ``filters`` below must agree with them to one
float32 rounding of the float64 design (libm's sin / cos / sqrt are not bit-identical between implementations).
"""
import numpy as np

import fp32_bounds as fb


def i0(x):
    q = x * x / 4.0
    term, total = 1.0, 1.0
    for j in range(1, 2000):
        term *= q / (j * j)
        total += term
        if term < 1e-18 * total:
            break
    return total


def kaiser(M, beta):
    alpha = (M - 1) / 2.0
    n = np.arange(M)
    r = (n - alpha) / alpha
    return np.array([i0(beta * np.sqrt(max(0.0, 1.0 - v * v))) for v in r]) / i0(beta)


def filters(K, taps, cutoff_ratio, beta):
    """-> (analysis, synthesis), float64 arrays (K, taps + 1) holding the float32-rounded values."""
    cutoff, beta = float(np.float32(cutoff_ratio)), float(np.float32(beta))
    n = np.arange(taps + 1)
    c = n - taps / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        proto = np.where(c == 0, cutoff, np.sin(np.pi * cutoff * c) / (np.pi * c)) * kaiser(taps + 1, beta)
    k = np.arange(K)[:, None]
    sgn = np.where(k % 2 == 0, 1.0, -1.0)
    ph = (2 * k + 1) * np.pi / (2.0 * K) * c[None, :]
    ana = 2.0 * proto[None, :] * np.cos(ph + sgn * np.pi / 4.0)
    syn = 2.0 * proto[None, :] * np.cos(ph - sgn * np.pi / 4.0)
    return ana.astype(np.float32).astype(np.float64), syn.astype(np.float32).astype(np.float64)


def filter_tolerance(ref):
    """What two correct float64 designs may differ by after rounding to float32: one float32 rounding of the value, plus the
    float64 evaluation's own error near a zero crossing (a few 1e-16 of the largest tap)."""
    return fb.U * 2.0 * np.abs(ref) + 1e-14


def analysis(x, ana, with_bound=True):
    """x (L,), ana (K, taps + 1) -> (bands (K, floor(L / K)), bound)."""
    x = np.asarray(x, np.float64)
    ana = np.asarray(ana, np.float64)
    K, N = ana.shape
    h, M = (N - 1) // 2, len(x) // K
    xp = np.concatenate([np.zeros(h), x, np.zeros(h + K)])
    idx = np.arange(M)[:, None] * K + np.arange(N)[None, :]
    W = xp[idx]                                                   # (M, N): W[m, n] = x[m K + n - h]
    bands = ana @ W.T
    if not with_bound:
        return bands, None
    return bands, fb.dot_bound(np.abs(ana) @ np.abs(W).T, N)


def nprod_synthesis(K, taps):
    return K * (-(-(taps + 1) // K))


def synthesis(bands, syn, with_bound=True):
    """bands (K, M), syn (K, taps + 1) -> (wav (K M,), bound)."""
    bands = np.asarray(bands, np.float64)
    syn = np.asarray(syn, np.float64)
    K, N = syn.shape
    h, M = (N - 1) // 2, bands.shape[1]
    T = K * M
    wav, ab = np.zeros(T), np.zeros(T)
    t = np.arange(T)
    for m in range(M):
        n = m * K - t + h
        ok = (n >= 0) & (n < N)
        wav[ok] += (syn[:, n[ok]] * bands[:, m][:, None]).sum(0)
        ab[ok] += (np.abs(syn[:, n[ok]]) * np.abs(bands[:, m])[:, None]).sum(0)
    wav *= K
    if not with_bound:
        return wav, None
    return wav, fb.dot_bound(K * ab, nprod_synthesis(K, N - 1))


def analysis_correlate(x, ana):
    """The definition, with numpy.correlate: zero-pad by taps / 2, correlate, take every K-th sample."""
    K, N = ana.shape
    h = (N - 1) // 2
    xp = np.pad(np.asarray(x, np.float64), (h, h))
    return np.stack([np.correlate(xp, ana[k], mode="valid")[::K][:len(x) // K] for k in range(K)])


def synthesis_correlate(bands, syn):
    """The definition: K - 1 zeros between samples, scaled by K, zero-padded by taps / 2, correlated, summed over k."""
    K, N = syn.shape
    h, M = (N - 1) // 2, bands.shape[1]
    out = np.zeros(K * M)
    for k in range(K):
        u = np.zeros(K * M)
        u[::K] = K * np.asarray(bands[k], np.float64)
        out += np.correlate(np.pad(u, (h, h)), syn[k], mode="valid")
    return out
