"""fp64 numpy restatement of the GE2E similarity matrix, softmax loss and EER labels
(parakeet/models/lstm_speaker_encoder.py:55-147), written from the formulas (a plain module, not a conftest).

    c_n      = mean_m e[n, m]                       inclusive centroid,  c^_n = c_n / |c_n|
    x[n, m]  = (sum_m' e[n, m'] - e[n, m]) / (M-1)  exclusive centroid,  x^ = x / |x|
    p1[r, j] = e_r . c^_j                           r = n M + m
    p2[r]    = e_r . x^_r
    p[r, j]  = (p2[r] if j == n(r) else p1[r, j]) * w + b
    term[r]  = logsumexp_j p[r, j] - p[r, n(r)],    loss = mean_r term[r]

It is the oracle of the GPU tests; tests/golden/ge2e_loss.npz (the reference's own source run over the Paddle stand-in,
tools/make_golden_ge2e_loss.py) pins it.  ``mutant`` selects a deliberately wrong variant, for the tests that show the
bounds of tests/ge2e_bounds.py reject them:
    "incl_diag"     the own-speaker column is not replaced (the inclusive centroid stays on the diagonal)
    "excl_nosub"    the exclusive centroid without the subtraction, sum_m' e / (M - 1)
    "no_wb"         w and b are not applied
    "target_shift"  the cross-entropy target is the next speaker
"""
import numpy as np

MUTANTS = ("incl_diag", "excl_nosub", "no_wb", "target_shift")


def own_speaker(N, M):
    return np.arange(N * M) // M


def similarity_matrix(embeds, w=10.0, b=-5.0, mutant=None):
    """embeds (N, M, C) -> p (N*M, N), p1 (N*M*N,), p2 (N*M,), all float64"""
    e = np.asarray(embeds, dtype=np.float64)
    N, M, C = e.shape
    c = e.mean(axis=1)
    c_hat = c / np.sqrt((c * c).sum(axis=1, keepdims=True))
    total = e.sum(axis=1, keepdims=True)
    x = (total - e if mutant != "excl_nosub" else np.broadcast_to(total, e.shape)) / (M - 1)
    x_hat = x / np.sqrt((x * x).sum(axis=2, keepdims=True))
    rows = e.reshape(N * M, C)
    p1 = rows @ c_hat.T
    p2 = (rows * x_hat.reshape(N * M, C)).sum(axis=1)
    p = p1.copy()
    if mutant != "incl_diag":
        p[np.arange(N * M), own_speaker(N, M)] = p2
    if mutant != "no_wb":
        p = p * float(w) + float(b)
    return p, p1.reshape(-1), p2


def row_terms(p, M, mutant=None):
    """p (N*M, N) -> (N*M,) logsumexp(p_row) - p_row[target]"""
    p = np.asarray(p, dtype=np.float64)
    NM, N = p.shape
    tgt = own_speaker(N, M)
    if mutant == "target_shift":
        tgt = (tgt + 1) % N
    mx = p.max(axis=1)
    lse = mx + np.log(np.exp(p - mx[:, None]).sum(axis=1))
    return lse - p[np.arange(NM), tgt]


def labels(N, M):
    """(N*M, N) one-hot speaker labels, the rows of inv_argmax (:139-140)"""
    y = np.zeros((N * M, N), dtype=np.int64)
    y[np.arange(N * M), own_speaker(N, M)] = 1
    return y


def loss(embeds, w=10.0, b=-5.0, mutant=None):
    """-> dict(p, p1, p2, terms, loss), float64"""
    M = np.shape(embeds)[1]
    p, p1, p2 = similarity_matrix(embeds, w, b, mutant)
    t = row_terms(p, M, mutant)
    return {"p": p, "p1": p1, "p2": p2, "terms": t, "loss": float(t.mean())}


def cosine(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(-1) / (np.sqrt((a * a).sum(-1)) * np.sqrt((b * b).sum(-1)))


def embeddings(N, M, C, seed, normalise=True, spread=1.0):
    """Strictly positive GE2E-shaped test embeddings, float32: relu-like noise + 0.01 plus a per-speaker offset (no
    centroid can vanish), unit rows unless ``normalise`` is False (then rows of very different lengths)."""
    rng = np.random.default_rng(seed)
    off = np.maximum(rng.standard_normal((N, 1, C)), 0.0) * spread
    e = np.maximum(rng.standard_normal((N, M, C)), 0.0) + 0.01 + off
    if normalise:
        e = e / np.sqrt((e * e).sum(-1, keepdims=True))
    else:
        e = e * np.exp(rng.normal(0.0, 1.0, size=(N, M, 1)))
    return e.astype(np.float32)
