"""The float64 restatement of parakeet_amd/csrc/pk_iir.h: the biquad recurrence, the plan of 256-sample
chunks with its transition matrix and carry, and gated loudness with its summation orders.  Change one, change the other.

Every operation is a separate IEEE float64 operation.  The chunks of the local and apply passes are independent, so numpy
carries them side by side (an elementwise numpy operation on float64 arrays is the scalar operation per element: numpy fuses
nothing); the carry over chunks and the per-sample order inside a chunk are loops, as the header writes them."""
import math

import numpy as np

CHUNK = 256
MAX_SECTIONS = 8
THREADS = 256
ABS = 1.1724653045822956e-07          # 10.0 ** -6.9309: -70 LUFS as a power
assert ABS == 10.0 ** -6.9309
SR_MIN, SR_MAX = 8000, 192000


def k_weighting(sr):
    """The two sections of BS.1770's K-weighting at rate sr, by libebur128's formulas, in Python floats."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, hp], dtype=np.float64)


def check_sos(sos):
    sos = np.asarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6 or not 1 <= sos.shape[0] <= MAX_SECTIONS:
        raise ValueError(f"sos of shape {sos.shape}")
    if not np.isfinite(sos).all() or (sos[:, 3] != 1.0).any():
        raise ValueError("a0 must be 1 and every coefficient finite")
    return sos


def run_chunks(sos, X, Z, n_valid=None):
    """X (C, T) float64 inputs of C independent chunks, Z (C, 2 S) their start states -> (outputs (C, T), end states).
    ``n_valid`` (C,): a chunk's state stops moving after that many samples (the partial last chunk)."""
    S = sos.shape[0]
    Z = np.array(Z, dtype=np.float64)
    Y = np.empty_like(X)
    for t in range(X.shape[1]):
        v = X[:, t]
        live = None if n_valid is None else t < n_valid
        for s in range(S):
            b0, b1, b2, _, a1, a2 = (float(c) for c in sos[s])
            o = b0 * v + Z[:, 2 * s]
            z0 = (b1 * v - a1 * o) + Z[:, 2 * s + 1]
            z1 = b2 * v - a2 * o
            Z[:, 2 * s] = z0 if live is None else np.where(live, z0, Z[:, 2 * s])
            Z[:, 2 * s + 1] = z1 if live is None else np.where(live, z1, Z[:, 2 * s + 1])
            v = o
        Y[:, t] = v
    return Y, Z


def transition(sos):
    """P (2 S, 2 S): column j = the end state of one chunk of zero input from the unit state e_j."""
    sos = check_sos(sos)
    n = 2 * sos.shape[0]
    _, Z = run_chunks(sos, np.zeros((n, CHUNK)), np.eye(n))
    return np.ascontiguousarray(Z.T)


def _chunked(x):
    """float32 signal -> (C, 256) float64, zeros behind the end; the samples of every chunk."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    L = x.shape[0]
    C = (L + CHUNK - 1) // CHUNK
    X = np.zeros((C, CHUNK), dtype=np.float64)
    X.reshape(-1)[:L] = x.astype(np.float64)
    n_valid = np.minimum(CHUNK, L - CHUNK * np.arange(C))
    return X, n_valid


def start_states(sos, X, nfull, P=None):
    """The carry pass: (C, 2 S) start states of all C chunks, nfull of which are full."""
    n = 2 * sos.shape[0]
    C = X.shape[0]
    P = transition(sos) if P is None else P
    _, q = run_chunks(sos, X[:nfull], np.zeros((nfull, n)))
    st = np.zeros((C, n), dtype=np.float64)
    s = [0.0] * n
    Pl = [[float(P[i, j]) for j in range(n)] for i in range(n)]
    for c in range(C):
        st[c] = s
        if c < nfull:
            ns = []
            for i in range(n):
                a = 0.0
                for j in range(n):
                    a = a + Pl[i][j] * s[j]
                ns.append(a + float(q[c, i]))
            s = ns
    return st


def sosfilt64(sos, x, P=None):
    """The plan of pk_iir.h on one float32 signal -> the float64 outputs, not yet rounded."""
    sos = check_sos(sos)
    X, n_valid = _chunked(x)
    L = np.asarray(x).shape[0]
    if L == 0:
        return np.zeros(0, dtype=np.float64)
    st = start_states(sos, X, L // CHUNK, P)
    Y, _ = run_chunks(sos, X, st, n_valid)
    return Y.reshape(-1)[:L].copy()


def sosfilt(sos, x, P=None):
    """... rounded once to float32: what ``audio.sosfilt`` returns."""
    return sosfilt64(sos, x, P).astype(np.float32)


def lfilter_sos(b, a):
    """One section from b, a of up to three coefficients, normalised by a[0] (what ``audio.lfilter`` builds)."""
    b, a = [float(v) for v in b], [float(v) for v in a]
    b, a = b + [0.0] * (3 - len(b)), a + [0.0] * (3 - len(a))
    return np.array([[b[0] / a[0], b[1] / a[0], b[2] / a[0], 1.0, a[1] / a[0], a[2] / a[0]]], dtype=np.float64)


def _tree(p, keep):
    """THE ORDER over blocks: item t adds the kept p_j, j = t, t + 256, ... ascending to 0.0, then the halving tree."""
    a = np.zeros(THREADS, dtype=np.float64)
    for r in range(0, len(p), THREADS):
        m = min(THREADS, len(p) - r)
        a[:m] = np.where(keep[r:r + m], a[:m] + p[r:r + m], a[:m])
    h = THREADS // 2
    while h >= 1:
        a[:h] = a[:h] + a[h:2 * h]
        h //= 2
    return float(a[0])


def segments(z, sr):
    """z: the float64 filtered samples -> seg (G,) by the pieces of the chunks, in the header's order."""
    h = sr // 10
    L = z.shape[0]
    G = L // h
    C = (L + CHUNK - 1) // CHUNK
    Zc = np.zeros((C, CHUNK), dtype=np.float64)
    Zc.reshape(-1)[:L] = z
    pos = CHUNK * np.arange(C)[:, None] + np.arange(CHUNK)[None, :]
    g0 = (CHUNK * np.arange(C)) // h
    first = pos < ((g0 + 1) * h)[:, None]
    valid = pos < L
    acc0, acc1 = np.zeros(C), np.zeros(C)
    for t in range(CHUNK):
        zz = Zc[:, t] * Zc[:, t]
        acc0 = np.where(valid[:, t] & first[:, t], acc0 + zz, acc0)
        acc1 = np.where(valid[:, t] & ~first[:, t], acc1 + zz, acc1)
    seg = np.zeros(G, dtype=np.float64)
    for g in range(G):
        acc = 0.0
        for c in range(g * h // CHUNK, ((g + 1) * h - 1) // CHUNK + 1):
            acc = acc + float(acc0[c] if g0[c] == g else acc1[c])
        seg[g] = acc
    return seg


def block_powers(seg, sr):
    h = sr // 10
    J = max(0, len(seg) - 3)
    if J == 0:
        return np.zeros(0, dtype=np.float64)
    return (((seg[0:J] + seg[1:J + 1]) + seg[2:J + 2]) + seg[3:J + 3]) / float(4 * h)


def check_sr(sr):
    if int(sr) != sr or sr % 10 != 0 or not SR_MIN <= sr <= SR_MAX:
        raise NotImplementedError(f"sr = {sr}")
    return int(sr)


def loudness(x, sr, sos=None):
    """dict(mean_power, gated, gated_abs, blocks, rel, peak, lufs, p): gated loudness of one float32 signal."""
    sr = check_sr(sr)
    sos = k_weighting(sr) if sos is None else sos
    x = np.asarray(x)
    z = sosfilt64(sos, x)
    p = block_powers(segments(z, sr), sr)
    k1 = p > ABS
    n1 = int(k1.sum())
    mean, rel, n2 = 0.0, 0.0, 0
    if n1 > 0:
        rel = 0.1 * (_tree(p, k1) / float(n1))
        k2 = k1 & (p > rel)
        n2 = int(k2.sum())
        if n2 > 0:
            mean = _tree(p, k2) / float(n2)
    peak = np.float32(np.abs(x).max()) if x.size else np.float32(0)
    lufs = -0.691 + 10.0 * np.log10(mean) if n2 > 0 else -np.inf
    return dict(mean_power=mean, gated=n2, gated_abs=n1, blocks=len(p), rel=rel, peak=peak, lufs=float(lufs), p=p)
