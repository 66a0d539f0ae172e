"""Feature statistics (csrc/pk_stats.h) restated in numpy float64 in the stated order, an extended-precision
two-pass value, the error bound the tests use and their corpora (a plain module, not a conftest).  Nothing here imports
parakeet_amd.

    state   n, K (float32, the first row ever seen or the caller's shift), S1 = sum (x - K), S2 = sum (x - K)^2 (float64)
    d       = float64(x) - float64(K); q = d * d; every sum a chain of single float64 additions starting at +0.0
    tile    R = tile_rows(D) rows anchored at the utterance's first row; CW = col_width(D) column slots, G = 256 / CW row
            slots; row slot g adds the tile's rows g, g + G, ... ascending; the slots meet in a halving tree
            (p[g] += p[g + s] for g < s; s = G / 2, ..., 1)
    U       an utterance's tiles added in ascending order; S = S + U_b left to right
    mean    = K + S1 / n; var = max(S2 - S1^2 / n, 0) / n; scale = sqrt(var), 1 where var <= n eps var + (n mean eps)^2

The error bound.  Write u = 2^-53, A1 = sum |x - K|, S2 = sum (x - K)^2 (exact), gamma_k = k u / (1 - k u).
 * d carries one rounding (the difference of two float32 need not fit 53 bits), q = d * d two of d's and one of its own.
 * A term reaches the state through a chain of additions whose length the order fixes: at most ceil(R / G) in its row slot,
   log2 G in the tree, the tiles of its utterance, and one per utterance folded into the state from its own on.  With h the
   longest such chain of the corpus (``chain_length``), every term of S1 is multiplied by at most (1 + u)^(h + 1), every
   term of S2 by at most (1 + u)^(h + 3) (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: the bound holds
   for any order with that depth):
       |S1^ - S1| <= E1 = gamma_{h+1} A1,        |S2^ - S2| <= E2 = gamma_{h+3} S2.
 * mean^ = fl(K + fl(S1^ / n)): |mean^ - mean| <= (E1 + u (A1 + E1)) / n + u |mean^|               (|S1^| <= A1 + E1).
 * var^ = fl(max(S2^ - fl(fl(S1^ S1^) / n), 0) / n).  |S1^2 - S1^2| <= 2 A1 E1 + E1^2; the product and the quotient add
   2 u (A1 + E1)^2 / n to first order (3 u taken); the subtraction u |numerator^| <= u (S2 + E2) (both operands are
   non-negative and the numerator is not above S2^); clamping at 0 moves the value towards the exact one, which is >= 0;
   the last division adds u var^.  By Cauchy-Schwarz A1^2 <= n S2, so every term is in n, u, A1 and S2:
       |var^ - var| <= (E2 + (2 A1 E1 + E1^2 + 3 u (A1 + E1)^2) / n + u (S2 + E2)) / n + u var^.
The extended-precision value is a two-pass mean / variance in np.longdouble (64-bit significand here, pairwise sums): its
own error is below 2^-60 relative and is not carried.  Reordering utterances or merging accumulators with different K changes
h and K, never the form of the bound; ``merge`` adds the re-shift's roundings (``merge_slack``).
"""
import math

import numpy as np

U = 2.0 ** -53
THREADS = 256
EPS64 = float(np.finfo(np.float64).eps)


# ---- geometry (csrc/pk_stats.h)
def col_width(D):
    cw = 1
    while cw < D and cw < 64:
        cw *= 2
    return cw


def tile_rows(D):
    cw = col_width(D)
    nc = -(-D // cw)
    r = 4096
    while r > 32 and r * cw * nc > 32768:
        r //= 2
    return r


# ---- the restatement
def _as_rows(x, D):
    x = np.asarray(x, dtype=np.float32)
    return x.reshape(-1, D)


def utterance_sums(x, K):
    """(U1, U2) of one utterance about K, in the stated order."""
    K = np.asarray(K, np.float32)
    D = K.size
    x = _as_rows(x, D)
    L = x.shape[0]
    u1, u2 = np.zeros(D), np.zeros(D)
    if L == 0:
        return u1, u2
    R, G = tile_rows(D), THREADS // col_width(D)
    nt = -(-L // R)
    it = -(-R // G)
    d = np.zeros((nt * it * G, D))                     # rows past the end add +0.0: a float64 accumulator that is never -0.0 keeps its bits
    d[:L] = x.astype(np.float64) - K.astype(np.float64)[None]
    q = d * d
    d, q = d.reshape(nt, it, G, D), q.reshape(nt, it, G, D)
    p1, p2 = np.zeros((nt, G, D)), np.zeros((nt, G, D))
    for i in range(it):                                # a row slot's rows, ascending
        p1 = p1 + d[:, i]
        p2 = p2 + q[:, i]
    s = G // 2
    while s >= 1:                                      # the halving tree over the row slots
        p1 = p1[:, :s] + p1[:, s:2 * s]
        p2 = p2[:, :s] + p2[:, s:2 * s]
        s //= 2
    for t in range(nt):                                # the tiles, ascending
        u1 = u1 + p1[t, 0]
        u2 = u2 + p2[t, 0]
    return u1, u2


class RefState:
    """The accumulator, on the host."""

    def __init__(self, D, shift=None):
        self.D = D
        self.n = 0
        self.K = None if shift is None else np.asarray(shift, np.float32).reshape(D).copy()
        self.S1, self.S2 = np.zeros(D), np.zeros(D)

    def update(self, utts):
        for x in utts:
            x = _as_rows(x, self.D)
            if x.shape[0] == 0:
                continue
            if self.K is None:
                self.K = x[0].copy()
            u1, u2 = utterance_sums(x, self.K)
            self.S1 = self.S1 + u1
            self.S2 = self.S2 + u2
            self.n += x.shape[0]
        return self

    def state_bytes(self):
        k = np.zeros(self.D, np.float32) if self.K is None else self.K
        return np.int64(self.n).tobytes() + k.tobytes() + self.S1.tobytes() + self.S2.tobytes()


def derive(n, K, S1, S2):
    """(mean, var, scale) in float64 as the definition forms them."""
    nf = np.float64(n)
    mean = np.asarray(K, np.float32).astype(np.float64) + S1 / nf
    var = np.maximum(S2 - S1 * S1 / nf, 0.0) / nf
    scale = np.sqrt(var)
    scale[var <= nf * EPS64 * var + (nf * mean * EPS64) ** 2] = 1.0
    return mean, var, scale


def stats_f32(n, K, S1, S2):
    mean, _, scale = derive(n, K, S1, S2)
    return np.stack([mean, scale]).astype(np.float32)


def state_bytes_of(fs):
    """The same byte string from a FeatureStats' state_dict."""
    sd = fs.state_dict()
    k = np.zeros(sd["dim"], np.float32) if sd["shift"] is None else np.asarray(sd["shift"], np.float32)
    return np.int64(sd["n"]).tobytes() + k.tobytes() + np.asarray(sd["s1"], np.float64).tobytes() + \
        np.asarray(sd["s2"], np.float64).tobytes()


# ---- extended precision and the bound
def exact(utts, D, K):
    """Two-pass mean / variance of the concatenated corpus and A1 = sum |x - K|, S2 = sum (x - K)^2 in np.longdouble."""
    x = np.concatenate([_as_rows(v, D) for v in utts], 0).astype(np.longdouble)
    n = x.shape[0]
    mean = x.sum(0) / n
    var = ((x - mean) ** 2).sum(0) / n
    dk = x - np.asarray(K, np.float32).astype(np.longdouble)[None]
    return n, mean, var, np.abs(dk).sum(0), (dk * dk).sum(0)


def chain_length(lens, D):
    """h: the longest chain of additions a term passes through on its way into the state."""
    R, G = tile_rows(D), THREADS // col_width(D)
    lens = [int(v) for v in lens]
    B = len(lens)
    h = 0
    for b, L in enumerate(lens):
        if L:
            h = max(h, -(-min(L, R) // G) + int(math.log2(G)) + -(-L // R) + (B - b))
    return h


def _gamma(k):
    return k * U / (1.0 - k * U)


def bounds(n, h, A1, S2, mean_hat, var_hat):
    """(bound on |mean^ - mean|, bound on |var^ - var|), per column; the derivation is in the module's docstring."""
    A1, S2 = np.asarray(A1, np.float64) * (1 + 2 ** -40), np.asarray(S2, np.float64) * (1 + 2 ** -40)   # rounded up from longdouble
    E1, E2 = _gamma(h + 1) * A1, _gamma(h + 3) * S2
    b_mean = (E1 + U * (A1 + E1)) / n + U * np.abs(mean_hat)
    b_var = (E2 + (2 * A1 * E1 + E1 * E1 + 3 * U * (A1 + E1) ** 2) / n + U * (S2 + E2)) / n + U * np.abs(var_hat)
    return b_mean, b_var


def ratio(err, bound):
    """max err / bound over the columns (0 / 0, an exact value under a zero bound, counts as 0)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def merge_slack(n_o, K_o, K_s, A1_o, S2_o):
    """What re-shifting n_o rows' sums from K_o to K_s adds (S1' = S1 + n delta, S2' = S2 + 2 delta S1 + n delta^2 in
    float64): one rounding of delta, and three resp. six roundings on terms bounded by A1 + n |delta| and
    S2 + 2 |delta| A1 + n delta^2 -> (err S1, err S2), to be divided by the merged n (and, for var, combined as the bound's
    E1 / E2)."""
    delta = np.abs(np.asarray(K_o, np.float64) - np.asarray(K_s, np.float64))
    m1 = np.asarray(A1_o, np.float64) + n_o * delta
    m2 = np.asarray(S2_o, np.float64) + 2 * delta * np.asarray(A1_o, np.float64) + n_o * delta * delta
    return 4 * U * m1, 8 * U * m2


# ---- corpora
PAIRS = {"neg5": (-5.0, 2.0), "pos5": (5.2, 0.3), "unit": (0.0, 1.0), "neg8": (-8.0, 3.0), "hostile": (1e4, 1e-2)}


def gaussian(rng, L, D, offset, spread):
    return (offset + spread * rng.standard_normal((L, D))).astype(np.float32)


def gpu_lengths(D):
    """The issue's lengths for dimension D: {0, 1, 2, R - 1, R, R + 1, 2 R + 1} and one utterance of about 40 R rows."""
    R = tile_rows(D)
    return [0, 1, 2, R - 1, R, R + 1, 2 * R + 1], 40 * R + 3


def corpus(D, kind, seed=0, lens=None):
    """A ragged corpus (list of (L, D) float32 arrays) of one of the kinds the GPU tests name."""
    rng = np.random.default_rng(seed * 7919 + D)
    if lens is None:
        short, long_ = gpu_lengths(D)
        lens = [int(rng.choice(short)) for _ in range(7)] + [long_]
        lens[int(rng.integers(1, 7))] = 0
        lens[0] = max(lens[0], 1)
    if kind in PAIRS:
        o, s = PAIRS[kind]
        return [gaussian(rng, L, D, o, s) for L in lens]
    if kind == "const_col":                           # column 0 constant everywhere
        out = [gaussian(rng, L, D, 5.2, 0.3) for L in lens]
        for x in out:
            x[:, 0] = np.float32(3.25)
        return out
    if kind == "const_per_utt":                       # column 0 constant within an utterance, not across
        out = [gaussian(rng, L, D, 5.2, 0.3) for L in lens]
        for i, x in enumerate(out):
            x[:, 0] = np.float32(1.5 + 0.25 * i)
        return out
    if kind == "outlier_first":                       # a silent first pitch token: 0, then values around 5.2
        out = [gaussian(rng, L, D, 5.2, 0.3) for L in lens]
        next(x for x in out if x.shape[0])[0] = 0.0
        return out
    if kind == "single_row":
        return [gaussian(rng, 1, D, 5.2, 0.3)]
    raise KeyError(kind)
