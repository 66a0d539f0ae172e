"""Viterbi tracking over the pitch estimator's candidates ("Viterbi tracking over candidates") restated in numpy
float64, a brute-force path search to check the restatement with, and the "hard signal" (a plain module, not a conftest).
Nothing here imports parakeet_amd.

The input is d' (frames, tau_max + 1) as ``pitch_ref.cmnd`` defines it -- float64, or the fp32 rows of the device -- and
tau_min, tau_max, sr, K (1 ... 8), theta_c, lambda, cu, sw:

    candidates   tau in [tau_min, tau_max - 1] with d'(tau) < d'(tau - 1), d'(tau) <= d'(tau + 1), d'(tau) < theta_c; the K smallest
                 by (d', tau), stored by ascending tau; an empty slot has lag 0 and cost +inf
    states       the K slots (obs = d' of the slot) and state K, unvoiced (obs = cu)
    transitions  slot p -> slot s: lambda |T[tau_s] - T[tau_p]|, T[tau] = log2(tau) in float64;  unvoiced -> unvoiced 0;
                 voiced <-> unvoiced sw
    recurrence   D_0[s] = obs_0[s];  D_i[s] = min_p (D_(i-1)[p] + tr(p, s)) + obs_i[s], ties to the smaller p, slots of cost
                 +inf skipped; the last state is the smallest s of minimal D, the score that D
    refinement   the lag of a frame is its state's (0 for unvoiced); f0 as pitch_ref refines it
"""
import itertools
import math

import numpy as np

import pitch_ref as pr

K_DEFAULT, THETA_C, LAMBDA, SWITCH = 8, 0.5, 1.0, 0.05
WEAK = ((0.30, 0.36), (0.80, 0.86), (1.20, 1.30))


def log_tau(tau_max):
    """T[0 ... tau_max]: log2(tau) from the C library, one call per lag (what the engine's host code calls); T[0] = 0."""
    return np.array([0.0] + [math.log2(t) for t in range(1, tau_max + 1)])


def candidates(dp, tau_min, tau_max, theta_c=THETA_C, K=K_DEFAULT):
    """-> lag (frames, K) int64, cost (frames, K) of dp's dtype.  The comparisons are made on dp's own values; theta_c is
    rounded to dp's dtype first (the device compares fp32 with fp32)."""
    nf = dp.shape[0]
    theta_c = dp.dtype.type(theta_c)
    lag = np.zeros((nf, K), np.int64)
    cost = np.full((nf, K), np.inf, dp.dtype)
    t = np.arange(tau_min, tau_max)
    for i in range(nf):
        r = dp[i]
        ts = t[(r[t] < r[t - 1]) & (r[t] <= r[t + 1]) & (r[t] < theta_c)]
        sel = np.sort(ts[np.lexsort((ts, r[ts]))[:K]])
        lag[i, :sel.size] = sel
        cost[i, :sel.size] = r[sel]
    return lag, cost


def transition(p, s, lag_prev, lag_cur, K, T, lam, sw):
    if s < K and p < K:
        return lam * abs(T[lag_cur[s]] - T[lag_prev[p]])
    if s == K and p == K:
        return 0.0
    return sw


def viterbi(lag, cost, T, lam, cu, sw):
    """-> (state per frame, lag per frame, score)"""
    nf, K = lag.shape
    S = K + 1
    obs = np.concatenate([cost.astype(np.float64), np.full((nf, 1), float(cu))], axis=1)
    D = obs[0].copy()
    bp = np.zeros((nf, S), np.int64)
    for i in range(1, nf):
        nd = np.full(S, np.inf)
        for s in range(S):
            if obs[i, s] == np.inf:
                continue
            best, arg = np.inf, 0
            for p in range(S):
                if D[p] == np.inf:
                    continue
                v = D[p] + transition(p, s, lag[i - 1], lag[i], K, T, lam, sw)
                if v < best:
                    best, arg = v, p
            nd[s] = best + obs[i, s]
            bp[i, s] = arg
        D = nd
    s = int(np.argmin(D))
    score = float(D[s])
    states = np.zeros(nf, np.int64)
    for i in range(nf - 1, -1, -1):
        states[i] = s
        s = bp[i, s]
    out = np.where(states < K, lag[np.arange(nf), np.minimum(states, K - 1)], 0)
    return states, out, score


def brute_force(lag, cost, T, lam, cu, sw):
    """Every state sequence, costed front to back in the recurrence's order of additions; the optimum under the tie rules is
    the sequence that is smallest when read from its last state backwards.  -> (states, score, how many sequences have that score)"""
    nf, K = lag.shape
    obs = np.concatenate([cost.astype(np.float64), np.full((nf, 1), float(cu))], axis=1)
    live = [[s for s in range(K + 1) if obs[i, s] != np.inf] for i in range(nf)]
    best, count = None, 0
    for seq in itertools.product(*live):
        d = obs[0, seq[0]]
        for i in range(1, nf):
            d = (d + transition(seq[i - 1], seq[i], lag[i - 1], lag[i], K, T, lam, sw)) + obs[i, seq[i]]
        key = (d, tuple(reversed(seq)))
        count = 1 if best is None or d < best[0] else count + (d == best[0])
        if best is None or key < best:
            best = key
    return np.array(list(reversed(best[1])), np.int64), float(best[0]), int(count)


def refine(dp, lagv, sr):
    """float64 on dp's values (fp32 rows: what the device does, to be rounded to fp32 once by the caller)"""
    f0 = np.zeros(len(lagv))
    for i, t in enumerate(lagv):
        if t == 0:
            continue
        a, b, c = float(dp[i, t - 1]), float(dp[i, t]), float(dp[i, t + 1])
        den = a - 2.0 * b + c
        d = (a - c) / (2.0 * den) if (a >= b and c >= b and den > 0) else 0.0
        f0[i] = sr / (t + d)
    return f0


def track(dp, sr, tau_min, tau_max, K=K_DEFAULT, theta_c=THETA_C, lam=LAMBDA, cu=0.1, sw=SWITCH):
    lag, cost = candidates(dp, tau_min, tau_max, theta_c, K)
    states, lagv, score = viterbi(lag, cost, log_tau(tau_max), lam, cu, sw)
    return dict(cand_lag=lag, cand_cost=cost, states=states, lag=lagv, score=score, f0=refine(dp, lagv, sr))


def hard_signal(sr, seed, seconds=pr.DUR):
    """float32: pitch_ref's contour and eight harmonics (0.9^h / h, gain 0.3, random phases, a 1e-3 noise floor), no silent or
    noise segments; the odd harmonics are scaled by 0.05 inside [0.30, 0.36), [0.80, 0.86) and [1.20, 1.30) s, that gain
    smoothed with a 10 ms boxcar."""
    rng = np.random.default_rng(seed)
    n = int(round(pr.DUR * sr))
    t = np.arange(n) / sr
    phase = 2 * np.pi * np.cumsum(pr.f0_true(t)) / sr
    ph0 = rng.uniform(0, 2 * np.pi, 8)
    g = np.ones(n)
    for a, b in WEAK:
        g[(t >= a) & (t < b)] = 0.05
    k = int(0.01 * sr)
    g = np.convolve(np.pad(g, k, mode="edge"), np.ones(k) / k, mode="same")[k:-k]
    x = sum((g if h % 2 else 1.0) * 0.9 ** h / h * np.sin(h * phase + ph0[h - 1]) for h in range(1, 9)) * 0.3
    x = x + 1e-3 * rng.standard_normal(n)
    return x[:int(round(seconds * sr))].astype(np.float32)


def gross_errors(f0, sr, hop, lo=0.05, hi=pr.DUR - 0.05):
    """-> (gross, unvoiced): boolean masks over the frames with centres in (lo, hi) s of the hard signal: voiced with
    |f0 / true - 1| > 1 %, and unvoiced"""
    f0 = np.asarray(f0, np.float64)
    tc = np.arange(f0.size) * hop / sr
    inside = (tc > lo) & (tc < hi)
    true = pr.f0_true(tc)
    voiced = f0 > 0
    return inside & voiced & (np.abs(f0 / true - 1.0) > 0.01), inside & ~voiced
