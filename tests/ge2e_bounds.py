"""Derived error bounds for the engine's GE2E similarity matrix and loss (csrc/spk_loss.hip) against the fp64 restatement
tests/ge2e_loss_ref.py, in the manner of tests/fp32_bounds.py (a plain module, not a conftest).

No constant here comes from an observed error: each is the unit roundoff u = 2^-24 of binary32 (2^-53 of binary64), a count
of roundings, or the derivative of the function the error is propagated through.  Sums are bounded for ANY summation order
(Higham (3.5)), so the bounds do not depend on how the kernel splits its work.  The embeddings, w and b are float32 numbers
taken as exact; everything is evaluated in float64 from them.

The chain, for embeds e (N, M, C), r = n M + m:
  S      = sum_m e                      M terms:              b_S  = gamma(M - 1) sum_m |e|
  c      = S / M                        one division:          b_c  = b_S / M + u (|c| + b_S / M)
  |c|    = sqrt(sum_c c^2)              see norm_bound
  c^     = c / |c|                      see unit_bound
  p1     = e . c^                       propagated + dot_bound(|e| . (|c^| + b_c^), C)
  d      = S - e                        the cancellation: S carries b_S ABSOLUTE, however small S - e is; one rounding
  x      = d / (M - 1)                  one division
  x^, p2 as c^, p1
  p      = s w + b                      s = p2 on the own-speaker column, p1 elsewhere; two roundings (one if fused)
  term   = logsumexp(p_row) - p_own     logsumexp is 1-Lipschitz in the maximum norm; float64 evaluation: lse64_bound
  loss   = mean(term)                   float64 fold, then one rounding to float32
"""
import numpy as np

from fp32_bounds import U, dot_bound

U64 = 2.0 ** -53


def gamma(k):
    """k roundings compounded: k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


def norm_bound(v, b_v):
    """n = sqrt(sum_c v_c^2) over the last axis from entries with absolute error b_v -> (n, bound).
    The perturbed vector's norm differs by at most |b_v|_2 (reverse triangle inequality).  The fp32 sum of C squares: one
    rounding per square and C - 1 per chain of additions, all terms positive, relative gamma(C + 1) whatever the order; the
    square root halves a relative error (first order; gamma(C + 1) instead of half of it is kept, which covers the second
    order), and sqrtf adds 2u (not assumed correctly rounded)."""
    v = np.asarray(v, np.float64)
    C = v.shape[-1]
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    h = np.sqrt((np.asarray(b_v, np.float64) ** 2).sum(-1, keepdims=True))
    return n, h + (gamma(C + 1) + 2.0 * U) * (n + h)


def unit_bound(v, b_v, n, b_n):
    """v / n from v (error b_v) and n (error b_n < n): |v'/n' - v/n| <= b_v / n' + |v| |1/n' - 1/n| <= b_v / n_lo + |v| b_n /
    (n n_lo), n_lo = n - b_n; the division itself 2u (not assumed correctly rounded) of the largest value it can return."""
    n_lo = n - b_n
    assert (n_lo > 0).all(), "a centroid too close to zero for a bound"
    b = b_v / n_lo + np.abs(v) * b_n / (n * n_lo)
    return b + 2.0 * U * (np.abs(v) / n + b)


def lse64_bound(p):
    """float64 evaluation of logsumexp(p_row) - p_own from float32 p (N columns), by running maximum and rescaled sum: per
    element a subtraction, an exponential (its argument's rounding is amplified by the argument, at most the row's spread), a
    product and an addition -- 4 roundings with a spare on a positive sum: relative (4 N + 16) (1 + spread) 2^-53 on the sum,
    which the logarithm turns into the same absolute error; log itself and the two final additions: 4 roundings of the
    largest magnitude in play."""
    p = np.asarray(p, np.float64)
    N = p.shape[1]
    spread = p.max(axis=1) - p.min(axis=1)
    return (4 * N + 16) * (1.0 + spread) * U64 + 4.0 * U64 * (3.0 * np.abs(p).max(axis=1) + np.log(N) + 1.0)


def lse32_bound(p):
    """The extra error of a FLOAT32 evaluation of logsumexp(p_row) - p_own (the reference's own arithmetic, not the
    engine's): the subtraction of the maximum u * spread turned relative by exp, expf 4u, a sum of N positive terms (N - 1) u,
    logf 4u of |log| <= log N, and two additions of magnitudes up to 3 max|p| + log N."""
    p = np.asarray(p, np.float64)
    N = p.shape[1]
    spread = p.max(axis=1) - p.min(axis=1)
    return (spread + N + 3) * U + 4.0 * U * np.log(N) + 2.0 * U * (3.0 * np.abs(p).max(axis=1) + np.log(N))


def bounds(embeds, w, b):
    """-> dict(p, p1, p2, terms, loss, loss_f32): absolute error bounds shaped like ge2e_loss_ref.loss()'s entries
    (loss: the float64 mean; loss_f32: after its rounding to float32)."""
    e = np.asarray(embeds, np.float64)
    N, M, C = e.shape
    w, b = float(w), float(b)
    a = np.abs(e)
    S = e.sum(axis=1)                                  # (N, C)
    b_S = gamma(M - 1) * a.sum(axis=1)
    c = S / M
    b_c = b_S / M + U * (np.abs(c) + b_S / M)
    n, b_n = norm_bound(c, b_c)
    c_hat = c / n
    b_chat = unit_bound(c, b_c, n, b_n)
    rows = a.reshape(N * M, C)
    b_p1 = rows @ b_chat.T + dot_bound(rows @ (np.abs(c_hat) + b_chat).T, C)
    # exclusive centroid: d = S - e inherits b_S in full (the cancellation), then one rounding of its own
    d = S[:, None, :] - e
    b_d = b_S[:, None, :] + U * (np.abs(d) + b_S[:, None, :])
    x = d / (M - 1)
    b_x = b_d / (M - 1) + U * (np.abs(x) + b_d / (M - 1))
    nx, b_nx = norm_bound(x, b_x)
    x_hat = x / nx
    b_xhat = unit_bound(x, b_x, nx, b_nx)
    b_p2 = (a * b_xhat).sum(-1).reshape(-1) + dot_bound((a * (np.abs(x_hat) + b_xhat)).sum(-1).reshape(-1), C)
    # p = s w + b
    p1 = e.reshape(N * M, C) @ c_hat.T
    p2 = (e * x_hat).sum(-1).reshape(-1)
    own = np.arange(N * M) // M
    s, b_s = p1.copy(), b_p1.copy()
    s[np.arange(N * M), own] = p2
    b_s[np.arange(N * M), own] = b_p2
    p = s * w + b
    prod = np.abs(w) * (np.abs(s) + b_s)               # the largest product the kernel can have formed
    b_p = np.abs(w) * b_s + U * prod
    b_p = b_p + U * (np.abs(p) + b_p)
    b_t = b_p.max(axis=1) + b_p[np.arange(N * M), own] + lse64_bound(p)
    mx = p.max(axis=1)
    terms = mx + np.log(np.exp(p - mx[:, None]).sum(axis=1)) - p[np.arange(N * M), own]
    b_loss = b_t.mean() + (N * M + 2) * U64 * np.abs(terms).mean()
    b_loss32 = b_loss + U * (abs(terms.mean()) + b_loss)
    return {"p": b_p, "p1": b_p1.reshape(-1), "p2": b_p2, "terms": b_t, "loss": b_loss, "loss_f32": b_loss32}


def cosine_bound(a, b):
    """a . b / (|a| |b|) of float32 rows: dot_bound on the numerator, norm_bound on the two norms, the product and the
    quotient 3u (the division not assumed correctly rounded)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    C = a.shape[-1]
    num = (a * b).sum(-1)
    b_num = dot_bound((np.abs(a) * np.abs(b)).sum(-1), C)
    na, b_na = norm_bound(a, np.zeros_like(a))
    nb, b_nb = norm_bound(b, np.zeros_like(b))
    na, nb, b_na, b_nb = na[..., 0], nb[..., 0], b_na[..., 0], b_nb[..., 0]
    den = na * nb
    b_den = na * b_nb + nb * b_na + b_na * b_nb
    den_lo = den - b_den
    bq = b_num / den_lo + np.abs(num) * b_den / (den * den_lo)
    return bq + 3.0 * U * (np.abs(num) / den + bq)
