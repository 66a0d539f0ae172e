"""fp64 numpy restatement of DESIGN.md 4.7: the monotonic alignment search, the attention-mode scores, the duration
post-step and the focus rate -- what ``parakeet_amd.alignment`` computes on the engine (csrc/align.hip, csrc/pk_align.h).

One utterance: S >= 1 rows (decoder steps), T columns (tokens), 1 <= T <= S, scores v[s, t] float32, higher is better.
Path: t(0) = 0, t(S - 1) = T - 1, t(s + 1) - t(s) in {0, 1}.
Forward, float64, every v converted exactly: Q(0, 0) = v(0, 0); Q(s, t) = v(s, t) + max(Q(s - 1, t), Q(s - 1, t - 1)) for
t <= s; Q(s, t) = -inf for t > s and for t = -1.  One IEEE addition per cell and no product: the engine agrees bit for bit.
Backtrack from (S - 1, T - 1): at row s >= 1 in column t stay iff Q(s - 1, t) >= Q(s - 1, t - 1) (ties stay), else t - 1.
status = 1 iff a v(s, t) with t <= s is not finite (durations then unspecified)."""
import itertools

import numpy as np


def mas(v):
    """(S, T) scores -> dict(durations int32 (T,), path int32 (S,), score float64, status int).  With status 1 only ``status``
    and ``score`` mean anything."""
    v = np.asarray(v)
    assert v.dtype == np.float32 and v.ndim == 2
    S, T = v.shape
    assert 1 <= T <= S
    s_idx, t_idx = np.arange(S)[:, None], np.arange(T)[None, :]
    status = int(not np.isfinite(v[t_idx <= s_idx]).all())
    x = v.astype(np.float64)
    Q = np.full((S, T), -np.inf)
    Q[0, 0] = x[0, 0]
    move = np.zeros((S, T), dtype=bool)                # at row s in column t: go to t - 1
    with np.errstate(invalid="ignore"):
        for s in range(1, S):
            up = Q[s - 1]
            left = np.concatenate(([-np.inf], Q[s - 1, :-1]))
            stay = up >= left
            move[s] = ~stay
            n = min(s, T - 1) + 1                      # columns t <= s
            Q[s, :n] = x[s, :n] + np.where(stay, up, left)[:n]
    path = np.zeros(S, dtype=np.int32)
    t = T - 1
    for s in range(S - 1, 0, -1):
        path[s] = t
        if move[s, t] and t > 0:
            t -= 1
    path[0] = t
    return dict(durations=np.bincount(path, minlength=T).astype(np.int32), path=path, score=Q[S - 1, T - 1], status=status)


def attention_scores_f64(att, eps=1e-8):
    """log(A < eps ? eps : A) in float64 (eps rounded to float32 first): what the engine's fp32 ``logf`` approximates."""
    a = np.asarray(att, dtype=np.float32)
    e = np.float32(eps)
    return np.log(np.where(a < e, e, a).astype(np.float64))


def post_step(durations, reduction_factor=1, merge_last=False):
    """``merge_last``: the last column's rows go to the column before it and the column is dropped (the <eos> column of a
    TransformerTTS map); then every count is multiplied by ``reduction_factor`` (a decoder step is r frames)."""
    d = np.asarray(durations, dtype=np.int32).copy()
    if merge_last:
        assert d.size >= 2
        d[-2] += d[-1]
        d = d[:-1]
    return d * np.int32(reduction_factor)


def focus_rate(att):
    """F = (1 / S) sum_s max_t A[s, t] of an (S, T) map (FastSpeech, 3.3): the maximum exact, the sum in float64."""
    a = np.asarray(att)
    assert a.dtype == np.float32 and a.ndim == 2
    return float(a.max(axis=1).astype(np.float64).sum() / a.shape[0])


def all_paths(S, T):
    """Every monotonic path of an S x T map as an (n, S) int array: the rows s >= 1 at which the column advances."""
    out = []
    for steps in itertools.combinations(range(1, S), T - 1):
        inc = np.zeros(S, dtype=np.int64)
        inc[list(steps)] = 1
        out.append(np.cumsum(inc))
    return np.asarray(out, dtype=np.int64).reshape(len(out), S)


def path_score(v, path):
    """The path's score summed as the forward pass sums it: row 0 first, one float64 addition per row."""
    x = np.asarray(v).astype(np.float64)
    q = x[0, path[0]]
    for s in range(1, len(path)):
        q = x[s, path[s]] + q
    return q


def decision_words(S, T):
    """32-bit decision words of an S x T utterance (pk_align.h): compared with ``pk_mas_lds_words`` they place a case on either
    side of the LDS / global switch."""
    return S * 2 * ((T + 63) // 64)
