"""The pitch estimator's definition in numpy float64, the reference's steps after it, the test signal and
the bounds the tests use (a plain module, not a conftest).  Nothing here imports parakeet_amd.

    frames = N // hop + 1;  frame i reads L = W + tau_max samples from s = i hop - L // 2, zeros outside the signal
    d(tau)  = sum_{j < W} (x[s + j] - x[s + j + tau])^2,  tau = 1 ... tau_max
    d'(tau) = d(tau) tau / c(tau),  c(tau) = d(1) + ... + d(tau)  (1 where c(tau) is not > 0);  d'(0) = 1
    tau0    = the smallest tau in [tau_min, tau_max - 1] with d'(tau) < theta; none: unvoiced (lag 0, f0 0)
    tau*    = tau0, + 1 while tau* + 1 <= tau_max - 1 and d'(tau* + 1) < d'(tau*)
    delta   = (a - c) / (2 (a - 2 b + c)) with a, b, c = d'(tau* - 1, tau*, tau* + 1) if a >= b, c >= b, a - 2 b + c > 0, else 0
    f0      = sr / (tau* + delta)
"""
import math

import numpy as np

U = 2.0 ** -24


def lags(sr, f0min, f0max):
    return max(2, int(math.floor(sr / f0max))), int(math.ceil(sr / f0min))


def n_frames(n, hop):
    return n // hop + 1


def cmnd(x, hop, tau_max, W=None):
    """(frames, tau_max + 1) float64 d'."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    W = 2 * tau_max if W is None else W
    L = W + tau_max
    nf = n_frames(x.size, hop)
    xp = np.concatenate([np.zeros(L // 2), x, np.zeros((nf - 1) * hop + L)])
    X = np.lib.stride_tricks.as_strided(xp, shape=(nf, L), strides=(hop * xp.strides[0], xp.strides[0]))
    d = np.zeros((nf, tau_max + 1))
    for tau in range(1, tau_max + 1):
        e = X[:, :W] - X[:, tau:tau + W]
        d[:, tau] = np.einsum("ij,ij->i", e, e)
    c = np.cumsum(d, axis=1)
    tau = np.arange(tau_max + 1, dtype=np.float64)[None, :]
    out = np.where(c > 0, d * tau / np.where(c > 0, c, 1.0), 1.0)
    out[:, 0] = 1.0
    return out


def _margin(a, b):
    """relative distance of two compared values: |a - b| / max(|a|, |b|); inf where both are 0 (a relative error keeps an
    exact zero exact, so the comparison of two zeros cannot come out differently)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = np.maximum(np.abs(a), np.abs(b))
    return np.where(m > 0, np.abs(a - b) / np.where(m > 0, m, 1.0), np.inf)


def pick(dp, sr, tau_min, tau_max, theta=0.1):
    """dp (frames, tau_max + 1) -> dict of per-frame arrays: lag (0 unvoiced), f0, delta, kappa = (a + 2b + c) / (a - 2b + c) (1
    where delta is 0) and margin: the smallest relative distance between the two sides of any comparison the picker made
    (d'(tau) >= theta before tau0, d'(tau0) < theta, every descent step and the stop, a >= b and c >= b of the refinement)."""
    nf = dp.shape[0]
    lag = np.zeros(nf, np.int64)
    f0 = np.zeros(nf)
    delta = np.zeros(nf)
    kappa = np.ones(nf)
    margin = np.full(nf, np.inf)
    for i in range(nf):
        r = dp[i]
        under = np.nonzero(r[tau_min:tau_max] < theta)[0]
        if under.size == 0:
            margin[i] = _margin(r[tau_min:tau_max], theta).min()
            continue
        t = tau_min + int(under[0])
        m = [_margin(r[tau_min:t + 1], theta).min()]
        while t + 1 <= tau_max - 1:
            m.append(float(_margin(r[t + 1], r[t])))
            if not r[t + 1] < r[t]:
                break
            t += 1
        a, b, c = r[t - 1], r[t], r[t + 1]
        m += [float(_margin(a, b)), float(_margin(c, b))]
        den = a - 2 * b + c
        if a >= b and c >= b and den > 0:
            delta[i] = (a - c) / (2 * den)
            kappa[i] = (a + 2 * b + c) / den
        lag[i], f0[i], margin[i] = t, sr / (t + delta[i]), min(m)
    return dict(lag=lag, f0=f0, delta=delta, kappa=kappa, margin=margin)


def track(x, sr, hop, f0min, f0max, theta=0.1, W=None):
    tau_min, tau_max = lags(sr, f0min, f0max)
    dp = cmnd(x, hop, tau_max, W)
    res = pick(dp, sr, tau_min, tau_max, theta)
    res["cmnd"] = dp
    return res


# ---- the reference's steps after the estimator (get_feats.py:99-153), restated
def continuous_f0(f0):
    f0 = np.asarray(f0, dtype=np.float64).copy()
    nz = np.nonzero(f0 != 0)[0]
    if nz.size == 0:
        return f0
    return np.interp(np.arange(f0.size), nz, f0[nz])       # constant outside the first / last voiced frame


def log_f0(f0):
    f0 = np.asarray(f0, dtype=np.float64).copy()
    nz = f0 != 0
    f0[nz] = np.log(f0[nz])
    return f0


def average(x, d):
    """(T, 1): the mean of x over every token's frames, 0 for a token of no frames"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    cum = np.concatenate([[0], np.cumsum(np.asarray(d, dtype=np.int64))])
    return np.array([x[a:b].mean() if x[a:b].size else 0.0 for a, b in zip(cum[:-1], cum[1:])]).reshape(-1, 1)


# ---- the test signal
DUR, N_SEG, SILENT, NOISE = 1.6, 10, (2, 7), (4, 9)


def f0_true(t):
    return 110.0 * 2.0 ** (1.3 * t / DUR) * (1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * t))


def segment_of(t):
    return np.minimum((np.asarray(t) / (DUR / N_SEG)).astype(np.int64), N_SEG - 1)


def make_signal(sr, seed, seconds=DUR):
    """float32, ``seconds`` (<= 1.6) of: eight harmonics (0.9^h / h, random phases, gain 0.3) of f0_true in the voiced segments,
    white noise (sigma 0.3) in segments 4 and 9, zeros in segments 2 and 7 (exact but for the 10 ms at either end that a fade
    reaches into); 20 ms raised-cosine cross-fades centred on the segment boundaries; a 1e-3 noise floor under tone and noise."""
    rng = np.random.default_rng(seed)
    n = int(round(DUR * sr))
    t = np.arange(n) / sr
    phase = 2 * np.pi * np.cumsum(f0_true(t)) / sr
    ph0 = rng.uniform(0, 2 * np.pi, 8)
    tone = sum(0.9 ** h / h * np.sin(h * phase + ph0[h - 1]) for h in range(1, 9)) * 0.3
    noise = 0.3 * rng.standard_normal(n)
    floor = 1e-3 * rng.standard_normal(n)
    seg = segment_of(t)
    silent, noisy = np.isin(seg, SILENT), np.isin(seg, NOISE)
    k = int(round(0.020 * sr)) // 2 * 2                     # the fade is centred on the boundary between two segments
    fade = np.hanning(k + 2)[1:-1]
    fade /= fade.sum()

    def smooth(ind):                                       # a 0 / 1 indicator with raised-cosine transitions of k samples
        return np.convolve(np.pad(ind.astype(np.float64), k, mode="edge"), fade, mode="same")[k:-k]
    g_tone, g_noise = smooth(~silent & ~noisy), smooth(noisy)
    inside = np.convolve(np.pad(silent.astype(np.float64), k, mode="edge"), np.ones(k + 1), mode="same")[k:-k] > k + 0.5
    x = np.where(inside, 0.0, tone * g_tone + noise * g_noise + floor * (g_tone + g_noise))
    return x[:int(round(seconds * sr))].astype(np.float32)


def frame_kinds(sr, hop, n):
    """per frame (centre i hop): 'v' voiced segment, 'n' noise, 's' silent; and the centre time"""
    tc = np.arange(n_frames(n, hop)) * hop / sr
    seg = segment_of(np.minimum(tc, DUR - 1e-9))
    kind = np.where(np.isin(seg, SILENT), "s", np.where(np.isin(seg, NOISE), "n", "v"))
    return kind, tc, seg


# ---- bounds
def eps_crude(W, tau_max):
    return 2.0 * (W + tau_max + 8) * U


def eps_d(W, tau_max):
    """Relative error of the kernel's d' (d, c are sums of non-negative terms, so every rounding is a relative one):
    d(tau): the difference is rounded once and squared (2u), the W FMAs of the chain round once each: gamma_(W + 2);
    c(tau): a sum, in whatever order, of at most tau_max such d: their gamma_(W + 2) and gamma_(tau_max) of its own;
    d * tau (tau is exact), / c: u and 2u (the division is not assumed correctly rounded).
    (2 (W + 2) + tau_max + 3) u, with 0.1 % for the second-order terms of (1 + u)^n at n <= 5000."""
    return 1.001 * (2 * (W + 2) + tau_max + 3) * U


def decided(res, eps):
    return res["margin"] > 4.0 * eps


def f0_tolerance(res, sr, eps):
    """sr / (tau + delta)^2 * (eps + 4u) kappa (1 + 2 |delta|) per frame (0 for unvoiced frames).  delta = (a - c) / (2 D),
    D = a - 2b + c, from a, b, c of relative error eps: |d delta| <= eps (a + c) / (2 D) + |delta| eps (a + 2b + c) / D <=
    eps kappa (1/2 + |delta|); the kernel refines in float64 and rounds sr / (tau + delta) once."""
    den = np.where(res["lag"] > 0, res["lag"] + res["delta"], 1.0)
    tol = sr / den ** 2 * (eps + 4 * U) * res["kappa"] * (1 + 2 * np.abs(res["delta"]))
    return np.where(res["lag"] > 0, tol, 0.0)
