"""The fp64 restatement of dynamic time warping (tests/dtw_ref.py) against brute force over every warping path,
the arithmetic of ``parakeet_amd.metrics`` on hand-made arrays, and the argument refusals of the Python layer (no GPU)."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dtw_ref as dr  # noqa: E402

_paths = {}


def _all_paths(N, M):
    if (N, M) not in _paths:
        _paths[N, M] = dr.all_paths(N, M)
    return _paths[N, M]


def _brute_q(c):
    """Q(i, j) by brute force: the smallest forward-order float64 sum over every warping path of c[:i + 1, :j + 1].  (Rounding
    is monotone, so the recurrence's Q is exactly this minimum.)"""
    N, M = c.shape
    Q = np.empty((N, M))
    for i in range(N):
        for j in range(M):
            Q[i, j] = min(dr.path_cost(c, [p[0] for p in path], [p[1] for p in path]) for path in _all_paths(i + 1, j + 1))
    return Q


def _rule_path(Q):
    """The path the tie rule selects, walked back on brute-force Q."""
    i, j = Q.shape[0] - 1, Q.shape[1] - 1
    out = [(i, j)]
    while i > 0 or j > 0:
        cand = [(Q[i - 1, j - 1] if i and j else np.inf, 0), (Q[i - 1, j] if i else np.inf, 1), (Q[i, j - 1] if j else np.inf, 2)]
        k = min(cand, key=lambda t: (t[0], t[1]))[1]   # the smallest; ties to the diagonal, then up, then left
        i, j = (i - 1, j - 1) if k == 0 else (i - 1, j) if k == 1 else (i, j - 1)
        out.append((i, j))
    return out[::-1]


@pytest.mark.parametrize("kind", ["random", "quantised"])
def test_restatement_against_brute_force(kind):
    rng = np.random.default_rng(3 if kind == "random" else 4)
    ties = 0
    for N in range(1, 7):
        for M in range(1, 7):
            c = (rng.standard_normal((N, M)) if kind == "random" else rng.integers(0, 3, size=(N, M))).astype(np.float32)
            ref = dr.dtw(c)
            costs = [dr.path_cost(c, [p[0] for p in path], [p[1] for p in path]) for path in _all_paths(N, M)]
            assert ref["cost"] == min(costs), (N, M)
            got = list(zip(ref["ix"].tolist(), ref["iy"].tolist()))
            assert got in [p for p, q in zip(_all_paths(N, M), costs) if q == min(costs)], (N, M)
            assert got == _rule_path(_brute_q(c)), (N, M)
            ties += sum(q == min(costs) for q in costs) > 1
            # the float64 sum of the path's costs in path order is the cost, bit for bit
            assert np.float64(dr.path_cost(c, ref["ix"], ref["iy"])).view(np.int64) == np.float64(ref["cost"]).view(np.int64)
            assert ref["length"] == len(got) and max(N, M) <= ref["length"] <= N + M - 1 and ref["status"] == 0
            assert ref["ix"].dtype == np.int32 and got[0] == (0, 0) and got[-1] == (N - 1, M - 1)
    assert ties > 5 if kind == "quantised" else True       # the tie rule did decide


def test_equal_costs_give_the_diagonal_and_the_straight_segment():
    """With all costs equal every tie goes to the diagonal: walked back from (N - 1, M - 1) the path is the pure diagonal
    followed by the remaining straight segment along row 0 (or column 0), as the tie rule dictates; in the forward order the
    path is returned in, the straight segment therefore comes first."""
    r = dr.dtw(np.full((3, 5), 0.25, np.float32))
    assert r["ix"].tolist() == [0, 0, 0, 1, 2] and r["iy"].tolist() == [0, 1, 2, 3, 4]
    assert r["ix"][::-1].tolist() == [2, 1, 0, 0, 0] and r["iy"][::-1].tolist() == [4, 3, 2, 1, 0]
    r = dr.dtw(np.full((5, 3), 0.25, np.float32))
    assert r["ix"].tolist() == [0, 1, 2, 3, 4] and r["iy"].tolist() == [0, 0, 0, 1, 2]
    assert r["cost"] == 1.25 and r["length"] == 5
    for N, M in ((4, 4), (1, 6), (6, 1), (2, 6)):
        r = dr.dtw(np.ones((N, M), np.float32))
        lead = abs(N - M)
        want_ix = [0] * lead + list(range(N)) if M >= N else list(range(N))
        want_iy = list(range(M)) if M >= N else [0] * lead + list(range(M))
        assert r["ix"].tolist() == want_ix and r["iy"].tolist() == want_iy and r["length"] == max(N, M)


def test_stretched_copy():
    rng = np.random.default_rng(5)
    for N, D in ((1, 3), (7, 1), (40, 13)):
        x = (np.arange(N)[:, None] * 3.0 + rng.random((N, D))).astype(np.float32)     # pairwise distinct rows
        d = rng.integers(1, 4, size=N)
        y = np.repeat(x, d, axis=0)
        r = dr.dtw_features(x, y)
        assert r["cost"] == 0.0 and np.array_equal(r["ix"], np.repeat(np.arange(N), d)) and np.array_equal(r["iy"], np.arange(len(y)))
        t = dr.dtw_features(y, x)                                                     # ... and the other way round
        assert t["cost"] == 0.0 and np.array_equal(t["iy"], np.repeat(np.arange(N), d)) and np.array_equal(t["ix"], np.arange(len(y)))


def test_status_and_local_cost_definition():
    c = np.ones((4, 5), np.float32)
    for v in (np.nan, np.inf):
        bad = c.copy()
        bad[2, 3] = v
        assert dr.dtw(bad)["status"] == 1
    assert dr.dtw(c)["status"] == 0
    x = np.array([[1e4, 1.0, 3e-4]], np.float32)
    y = np.array([[0.0, 0.5, 0.0]], np.float32)
    c, s = dr.local_cost(x, y, return_s=True)
    want = ((0.0 + float(x[0, 0]) ** 2) + 0.25) + float(x[0, 2]) ** 2
    assert s[0, 0] == want and c[0, 0] == np.float32(want)
    assert dr.local_cost(x, y, 1, 2)[0, 0] == np.float32(0.25)


def test_path_stats_restatement():
    rng = np.random.default_rng(6)
    x, y = rng.standard_normal((300, 5)).astype(np.float32), rng.standard_normal((280, 5)).astype(np.float32)
    r = dr.dtw_features(x, y, 1, 4)
    mx, my = rng.random(300) < 0.7, rng.random(280) < 0.7
    st = dr.path_stats(r["ix"], r["iy"], x, y, 1, 4, mx, my)
    s = ((x[r["ix"], 1:4].astype(np.float64) - y[r["iy"], 1:4].astype(np.float64)) ** 2).sum(axis=1)
    both = mx[r["ix"]] & my[r["iy"]]
    assert abs(st["sum_sq"] - s[both].sum()) <= 1e-12 * s[both].sum()
    assert abs(st["sum_sqrt"] - np.sqrt(s[both]).sum()) <= 1e-12 * np.sqrt(s[both]).sum()
    assert st["counts"].sum() == r["length"] and st["counts"][0] == both.sum()
    plain = dr.path_stats(r["ix"], r["iy"], x, y, 1, 4)
    assert plain["counts"].tolist() == [r["length"], 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------- the metrics
def test_dct_matrix_is_orthonormal():
    from parakeet_amd import metrics as mt
    for n in (1, 8, 80):
        w = mt.dct_matrix(n, n - 1)
        wl = w.astype(np.longdouble)                      # the Gram matrix in extended precision: the check adds no error of its own
        assert w.dtype == np.float64 and np.abs(wl.T @ wl - np.eye(n)).max() <= 1e-15
        assert np.array_equal(mt.dct_matrix(n, min(13, n - 1)), w[:, :min(13, n - 1) + 1])
        assert np.abs(w - dr.dct_matrix(n, n - 1)).max() <= 1e-14               # the plain formula
    m = mt.cepstrum_matrix(80, 13, 10.0)
    assert m.dtype == np.float32 and m.shape == (80, 14)
    assert np.array_equal(m, (math.log(10.0) * mt.dct_matrix(80, 13)).astype(np.float32))
    with pytest.raises(ValueError, match="n_coef"):
        mt.dct_matrix(8, 8)
    with pytest.raises(ValueError, match="log_base"):
        mt.cepstrum_matrix(8, 3, 1.0)


def test_mcd_of_a_hand_made_pair_against_the_formula():
    from parakeet_amd import metrics as mt
    rng = np.random.default_rng(7)
    ref, syn = rng.standard_normal((2, 8)).astype(np.float32), rng.standard_normal((2, 8)).astype(np.float32)
    w = mt.cepstrum_matrix(8, 3, 10.0).astype(np.float64)
    cr, cs = (ref.astype(np.float64) @ w).astype(np.float32), (syn.astype(np.float64) @ w).astype(np.float32)
    r = dr.dtw_features(cr, cs, 1, 4)
    st = dr.path_stats(r["ix"], r["iy"], cr, cs, 1, 4)
    got = mt.mcd_result(st["sum_sqrt"], r["length"], 2, 2)
    dist = lambda i, j: math.sqrt(sum((float(cr[i, k]) - float(cs[j, k])) ** 2 for k in range(1, 4)))  # noqa: E731
    steps = list(zip(r["ix"].tolist(), r["iy"].tolist()))
    want = 10.0 / math.log(10.0) * math.sqrt(2.0) * sum(dist(i, j) for i, j in steps) / len(steps)
    assert steps[0] == (0, 0) and steps[-1] == (1, 1) and abs(got["mcd"] - want) <= 1e-14 * want
    assert got["mcd"] == dr.mcd_db(st["sum_sqrt"], r["length"])
    assert got["length"] == len(steps) and got["rows"] == 2 and got["cols"] == 2 and got["length_ratio"] == 1.0
    # a copy: 0 dB
    same = dr.path_stats(*[dr.dtw_features(cr, cr, 1, 4)[k] for k in ("ix", "iy")], cr, cr, 1, 4)
    assert mt.mcd_result(same["sum_sqrt"], 2, 2, 2)["mcd"] == 0.0
    assert mt.mcd_result(1.0, 4, 2, 3)["length_ratio"] == 1.5


def test_f0_arithmetic_on_hand_made_arrays():
    from parakeet_amd import metrics as mt
    ref = np.array([0.0, 100.0, 110.0, 120.0, 0.0, 130.0, 140.0])
    syn = np.where(ref > 0, ref * 2.0 ** (1.0 / 12.0), 0.0)
    syn[1], syn[4] = 0.0, 90.0                              # one V -> UV, one UV -> V
    v_r, v_s = ref > 0, syn > 0
    both = v_r & v_s
    lr, ls = np.log(ref[both]), np.log(syn[both])
    sum_sq = float(((lr - ls) ** 2).sum())
    n11, n10, n01 = int(both.sum()), int((v_r & ~v_s).sum()), int((~v_r & v_s).sum())
    got = mt.f0_result(sum_sq, n11, n10, n01, 7)
    assert abs(got["f0_rmse_cents"] - 100.0) <= 1e-11 and abs(got["f0_rmse"] - math.log(2.0) / 12.0) <= 1e-15
    assert got["vuv_error"] == 2 / 7 and got["voiced_both"] == 4
    # ... and through the restatement's sums along a path (float32 logarithms: the rounding of the inputs is what is left)
    x, y = np.where(v_r, np.log(np.where(v_r, ref, 1.0)), 0.0).astype(np.float32)[:, None], \
        np.where(v_s, np.log(np.where(v_s, syn, 1.0)), 0.0).astype(np.float32)[:, None]
    st = dr.path_stats(np.arange(7), np.arange(7), x, y, 0, 1, v_r, v_s)
    assert st["counts"].tolist() == [4, 1, 1, 1]
    via = mt.f0_result(st["sum_sq"], *st["counts"][:3], 7)
    assert abs(via["f0_rmse_cents"] - 100.0) <= 1200.0 / math.log(2.0) * 2 * 2.0 ** -24 * math.log(140.0 * 1.06)
    none = mt.f0_result(0.0, 0, 3, 4, 7)
    assert math.isnan(none["f0_rmse"]) and math.isnan(none["f0_rmse_cents"]) and none["vuv_error"] == 1.0


# ----------------------------------------------------------------------------------- refusals of the Python layer (no engine)
def test_python_layer_refusals():
    from parakeet_amd import alignment as al
    from parakeet_amd import metrics as mt
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    with pytest.raises(NotImplementedError, match="4097 rows.*4096"):
        al.dtw(z(4097, 2))
    with pytest.raises(NotImplementedError, match="pair 1 has 4097 columns"):
        al.dtw([z(2, 2), z(2, 4097)])
    with pytest.raises(ValueError, match="empty"):
        al.dtw(z(0, 3))
    with pytest.raises(ValueError, match="no utterances"):
        al.dtw([])
    with pytest.raises(ValueError, match="rows and cols go together"):
        al.dtw(z(2, 3, 3), rows=[1, 2])
    with pytest.raises(ValueError, match="do not lie in"):
        al.dtw(z(2, 3, 3), rows=[1, 4], cols=[1, 1])
    with pytest.raises(NotImplementedError, match="feature dimension 129"):
        al.dtw_features(z(3, 129), z(2, 129))
    with pytest.raises(NotImplementedError, match="4097 rows"):
        al.dtw_features(z(4097, 2), z(2, 2))
    with pytest.raises(ValueError, match=r"columns \[5, 5\)"):
        al.dtw_features(z(3, 8), z(2, 8), (5, 5))
    with pytest.raises(ValueError, match=r"columns \[0, 9\)"):
        al.dtw_features(z(3, 8), z(2, 8), (0, 9))
    with pytest.raises(ValueError, match="x has 8 feature columns, y has 7"):
        al.dtw_features(z(3, 8), z(2, 7))
    with pytest.raises(ValueError, match="2 sequences x, 1 sequences y"):
        al.dtw_features([z(3, 8), z(3, 8)], [z(2, 8)])
    with pytest.raises(ValueError, match="x 1 is empty"):
        al.dtw_features([z(3, 8), z(0, 8)], [z(2, 8), z(2, 8)])
    with pytest.raises(ValueError, match="expected features of shape"):
        al.dtw_features(z(3), z(2))
    with pytest.raises(ValueError, match="y: lengths"):
        al.dtw_features(z(2, 3, 4), z(2, 3, 4), x_lens=[1, 2], y_lens=[1, 4])
    with pytest.raises(ValueError, match="2 reference log-mels, 1 synthesised"):
        mt.mcd_batch([z(3, 8), z(3, 8)], [z(2, 8)])
    with pytest.raises(ValueError, match="n_coef"):
        mt.mcd_batch(z(3, 8), z(2, 8), n_coef=0)
    with pytest.raises(ValueError, match="1 paths, 2 reference f0 tracks"):
        mt.f0_batch([al.DTWPath(None, None, 0.0, 1, 1, 1)], [z(1), z(1)], [z(1), z(1)])
    with pytest.raises(ValueError, match="reference signals"):
        mt.score_batch([z(10)], [], 24000)
    assert set(("dtw", "dtw_features", "path_stats")) <= set(al.__all__)
