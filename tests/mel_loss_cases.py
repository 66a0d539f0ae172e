"""The pairs of mel-like images the SSIM / masked-L1 tests and tools/make_golden_speedyspeech_forward.py share.

A case is (W, L, padded rows beyond L, window_size, kind).  Together the cases cover W in {1, 5, 80}, L in {1, 7, row tile - 1,
row tile, row tile + 1, 2 row tiles + 3}, padding in {0, 1, window_size // 2, 13} and window sizes {1, 3, 11}; none has fewer
than five valid entries, so that a case's largest deviation is that of several pixels and not the luck of one.  Two kinds of
input: "z" is z-scored (targets N(0, 1), predictions 10 % noise on them), "raw" is log-mel-like (mean -6, deviation 2, the same
relative noise).  Inputs are seeded by the case's name; nothing else is random."""
import collections
import zlib

import numpy as np

ROW_TILE = 16          # parakeet_amd._capi.PK_MEL_LOSS_ROWS (tests/test_mel_loss_cpu.py checks the two agree)
Case = collections.namedtuple("Case", "W L pad ws kind")

_SHAPES = [
    (80, 2 * ROW_TILE + 3, 0, 11), (80, ROW_TILE, 13, 11), (80, ROW_TILE + 1, 5, 11), (80, ROW_TILE - 1, 1, 11),
    (80, 7, 0, 3), (80, 1, 13, 11), (80, ROW_TILE, 0, 1),
    (5, 2 * ROW_TILE + 3, 1, 11), (5, ROW_TILE, 0, 3), (5, 7, 5, 11), (5, 1, 5, 11), (5, ROW_TILE + 1, 0, 1),
    (1, ROW_TILE + 1, 13, 3), (1, ROW_TILE - 1, 0, 11), (1, 2 * ROW_TILE + 3, 1, 3), (1, ROW_TILE, 0, 1),
]
CASES = [Case(*s, kind) for kind in ("z", "raw") for s in _SHAPES]


def case_id(c):
    return f"w{c.W}_l{c.L}_p{c.pad}_k{c.ws}_{c.kind}"


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def pair(c):
    """(pred, target) float32 (L, W)."""
    g = rng_for(case_id(c))
    mean, dev = (0.0, 1.0) if c.kind == "z" else (-6.0, 2.0)
    target = (mean + dev * g.standard_normal((c.L, c.W))).astype(np.float32)
    pred = (target + 0.1 * dev * g.standard_normal((c.L, c.W))).astype(np.float32)
    return pred, target


def padded(x, rows):
    """(L, W) -> (rows, W) with zero rows below: what ``x * spec_mask`` is in a batch padded to ``rows``."""
    out = np.zeros((rows, x.shape[1]), x.dtype)
    out[:x.shape[0]] = x
    return out
