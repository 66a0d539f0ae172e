"""fp64 numpy restatement of DESIGN.md 4.7b: dynamic time warping and the statistics along its path -- what
``parakeet_amd.alignment.dtw`` / ``dtw_features`` / ``path_stats`` compute on the engine (csrc/dtw.hip, csrc/pk_dtw.h).

One pair: N >= 1 rows (frames of x), M >= 1 columns (frames of y).
Local cost, matrix mode: c(i, j) is a given float32.  Feature mode: x (N, D), y (M, D) float32 and a column range [k0, k1);
s = 0.0; for k ascending: d = (double)x[i, k] - (double)y[j, k], s = s + d * d (separate float64 operations, no fused
multiply-add); c(i, j) = (float)s.
Forward, float64: Q(0, 0) = c(0, 0); Q(i, j) = c(i, j) + min(Q(i - 1, j - 1), Q(i - 1, j), Q(i, j - 1)), +inf outside.
The predecessor of (i, j) is the smallest of the three, ties to the diagonal first, then to (i - 1, j), then to (i, j - 1); in
row 0 it is (0, j - 1) and in column 0 it is (i - 1, 0) whatever the values are.  The path runs forward from (0, 0) to
(N - 1, M - 1).  status = 1 iff some c is not finite (the path is then unspecified)."""
import numpy as np

STATS_THREADS = 256                       # csrc/pk_dtw.h: DTW_STATS_THREADS


def local_cost(x, y, k0=0, k1=None, return_s=False):
    """(N, D), (M, D) float32 -> the (N, M) float32 cost matrix (and the float64 s before its rounding).  The loop over k is
    the definition: ``np.sum`` sums pairwise."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == np.float32 and y.dtype == np.float32 and x.ndim == 2 and y.ndim == 2 and x.shape[1] == y.shape[1]
    k1 = x.shape[1] if k1 is None else k1
    assert 0 <= k0 < k1 <= x.shape[1]
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    s = np.zeros((x.shape[0], y.shape[0]))
    with np.errstate(all="ignore"):
        for k in range(k0, k1):
            d = xd[:, k][:, None] - yd[:, k][None, :]
            dd = d * d
            s = s + dd
        c = s.astype(np.float32)
    return (c, s) if return_s else c


def dtw(c):
    """(N, M) float32 costs -> dict(ix, iy int32 (P,), length, cost float64, status).  Vectorised over anti-diagonals."""
    c = np.asarray(c)
    assert c.dtype == np.float32 and c.ndim == 2 and min(c.shape) >= 1
    N, M = c.shape
    status = int(not np.isfinite(c).all())
    x = c.astype(np.float64)
    Q = np.full((N + 1, M + 1), np.inf)                # Q[i + 1, j + 1] = Q(i, j)
    dec = np.zeros((N, M), dtype=np.int8)              # 0 diagonal, 1 up, 2 left
    Q[1, 1] = x[0, 0]
    with np.errstate(invalid="ignore"):
        for t in range(1, N + M - 1):
            i = np.arange(max(0, t - M + 1), min(N - 1, t) + 1)
            j = t - i
            d, u, lf = Q[i, j], Q[i, j + 1], Q[i + 1, j]
            m, k = d.copy(), np.zeros(i.size, dtype=np.int8)
            up = u < m
            m[up], k[up] = u[up], 1
            left = lf < m
            m[left], k[left] = lf[left], 2
            Q[i + 1, j + 1] = x[i, j] + m
            dec[i, j] = k
    i, j = N - 1, M - 1
    ix, iy = [i], [j]
    while i > 0 or j > 0:
        k = 2 if i == 0 else 1 if j == 0 else int(dec[i, j])
        if k == 0:
            i, j = i - 1, j - 1
        elif k == 1:
            i -= 1
        else:
            j -= 1
        ix.append(i)
        iy.append(j)
    return dict(ix=np.array(ix[::-1], dtype=np.int32), iy=np.array(iy[::-1], dtype=np.int32), length=len(ix), cost=Q[N, M],
                status=status)


def dtw_features(x, y, k0=0, k1=None):
    return dtw(local_cost(x, y, k0, k1))


def path_cost(c, ix, iy):
    """The path's cost summed as the forward pass sums it: (0, 0) first, one float64 addition per step."""
    x = np.asarray(c).astype(np.float64)
    q = x[ix[0], iy[0]]
    for p in range(1, len(ix)):
        q = x[ix[p], iy[p]] + q
    return q


def _fold(terms):
    """THE ORDER of pk_dtw.h: work item t adds the terms of steps t, t + T, t + 2 T, ... ascending to 0.0; then for
    h = T / 2, T / 4, ..., 1: a_t = a_t + a_(t + h) for t < h."""
    T = STATS_THREADS
    n = (len(terms) + T - 1) // T * T
    rows = np.zeros(n)
    rows[:len(terms)] = terms
    a = np.zeros(T)
    for row in rows.reshape(-1, T):
        a = a + row
    h = T // 2
    while h >= 1:
        a[:h] = a[:h] + a[h:2 * h]
        h //= 2
    return a[0]


def path_stats(ix, iy, x, y, k0=0, k1=None, mask_x=None, mask_y=None):
    """-> dict(sum_sq, sum_sqrt float64, counts int64 (n11, n10, n01, n00)).  s_p is the float64 s of step p before its
    rounding to float32; the sums run over the steps whose two masks are set, the counts over all steps."""
    x, y = np.asarray(x), np.asarray(y)
    k1 = x.shape[1] if k1 is None else k1
    ix, iy = np.asarray(ix, dtype=np.int64), np.asarray(iy, dtype=np.int64)
    xd, yd = x.astype(np.float64)[ix], y.astype(np.float64)[iy]
    s = np.zeros(len(ix))
    with np.errstate(all="ignore"):
        for k in range(k0, k1):
            d = xd[:, k] - yd[:, k]
            dd = d * d
            s = s + dd
        vx = np.ones(len(ix), bool) if mask_x is None else np.asarray(mask_x)[ix] != 0
        vy = np.ones(len(iy), bool) if mask_y is None else np.asarray(mask_y)[iy] != 0
        both = vx & vy
        sq = _fold(np.where(both, s, 0.0))
        rt = _fold(np.where(both, np.sqrt(s), 0.0))
    counts = np.array([(vx & vy).sum(), (vx & ~vy).sum(), (~vx & vy).sum(), (~vx & ~vy).sum()], dtype=np.int64)
    return dict(sum_sq=sq, sum_sqrt=rt, counts=counts)


def all_paths(N, M):
    """Every warping path of an N x M matrix: lists of (i, j) from (0, 0) to (N - 1, M - 1), steps (1, 1), (1, 0), (0, 1)."""
    out = []

    def walk(i, j, acc):
        acc = acc + [(i, j)]
        if i == N - 1 and j == M - 1:
            out.append(acc)
            return
        if i + 1 < N and j + 1 < M:
            walk(i + 1, j + 1, acc)
        if i + 1 < N:
            walk(i + 1, j, acc)
        if j + 1 < M:
            walk(i, j + 1, acc)

    walk(0, 0, [])
    return out


def decision_words(N, M):
    """32-bit decision words of an N x M pair (pk_dtw.h): compared with ``pk_dtw_lds_words`` they place a case on either side
    of the LDS / global switch."""
    R = 1
    while R < 16 and 64 * R < N:
        R *= 2
    return M * ((N + R - 1) // R)


# ------------------------------------------------------------------------------------------- the metrics (metrics.py)
def dct_matrix(n_mels, n_coef):
    """(n_mels, n_coef + 1) float64: column k is the orthonormal DCT-II basis vector k."""
    n = np.arange(n_mels, dtype=np.float64)[:, None]
    k = np.arange(n_coef + 1, dtype=np.float64)[None, :]
    w = np.cos(np.pi * (n + 0.5) * k / n_mels) * np.sqrt(2.0 / n_mels)
    w[:, 0] *= np.sqrt(0.5)
    return w


def mcd_db(sum_sqrt, P):
    return 10.0 / np.log(10.0) * np.sqrt(2.0) * sum_sqrt / P
