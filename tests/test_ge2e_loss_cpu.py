"""GE2E similarity matrix, loss and EER without a GPU: the fp64 restatement (tests/ge2e_loss_ref.py) against the reference's
own source (tests/golden/ge2e_loss.npz, tools/make_golden_ge2e_loss.py), ``equal_error_rate`` against the goldens and the
sklearn / scipy pipeline it restates, and the bounds of tests/ge2e_bounds.py against mutants of the restatement.

Bars.  The goldens' p, p1, p2 and loss were computed by the stand-in in float64 (the tool hands float64 embeddings over
and asserts the dtype), so the restatement is held to 1e-12 relative.  ``forward``'s own loss is the stand-in's float32
arithmetic on float32 embeddings: its bar is the derived fp32 bound of ge2e_bounds (valid for any summation order) plus
lse32_bound for the float32 cross-entropy.  The EER bar 1e-9 is far above brentq's xtol of 2e-12, the pipeline's own error."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ge2e_bounds as gb  # noqa: E402
import ge2e_loss_ref as ref  # noqa: E402
from fp32_bounds import ratio  # noqa: E402

from parakeet_amd.lstm_speaker_encoder import GE2EShapeError, equal_error_rate  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ge2e_loss.npz")
CASES = ["a", "b", "wb", "fwd"]


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(np.asarray(want)).max())


@pytest.mark.parametrize("name", CASES)
def test_restatement_vs_reference_golden(name):
    g = np.load(GOLD)
    assert list(g["case_names"]) == CASES
    e = g[f"{name}_embeds"]
    w, b = g[f"{name}_wb"]
    r = ref.loss(e, w, b)
    for k in ("p", "p1", "p2"):
        assert g[f"{name}_{k}"].dtype == np.float64 and g[f"{name}_{k}"].shape == r[k].shape
        assert _rel(r[k], g[f"{name}_{k}"]) < 1e-12, k
    assert abs(r["loss"] - float(g[f"{name}_loss"])) < 1e-12 * abs(float(g[f"{name}_loss"]))
    N, M, _ = e.shape
    assert abs(equal_error_rate(ref.labels(N, M), r["p"]) - float(g[f"{name}_eer"])) < 1e-9


def test_golden_cases_cover_the_parameters_and_the_literal_reshape():
    g = np.load(GOLD)
    assert tuple(g["wb_wb"]) == (7.5, -2.0) and tuple(g["a_wb"]) == (10.0, -5.0)
    N = int(g["fwd_num_speakers"])
    assert g["fwd_embeds"].shape == (N, g["fwd_seqs"].size // (N * N), N)
    assert np.array_equal(g["fwd_embeds"], g["fwd_seqs"].reshape(N, -1, N))
    norms = np.sqrt((g["fwd_embeds"].astype(np.float64) ** 2).sum(-1))
    assert norms.max() < 0.9, "the literal reshape feeds slices of unit vectors, not unit vectors"


def test_forward_float32_loss_of_the_reference_within_the_fp32_bound():
    g = np.load(GOLD)
    e = g["fwd_embeds"]
    r = ref.loss(e, 10.0, -5.0)
    bd = gb.bounds(e, 10.0, -5.0)
    bar = bd["loss_f32"] + float(gb.lse32_bound(r["p"]).mean())
    err = abs(float(g["fwd_forward_loss32"]) - r["loss"])
    print(f"forward fp32 loss: error {err:.3e}, bound {bar:.3e}")
    assert err <= bar


# ------------------------------------------------------------------------------------------------------------- EER
def _score_sets():
    """GE2E-shaped score sets: the restatement's similarity matrix of seeded embeddings with its one-hot labels."""
    shapes = [(2, 2, 1), (3, 2, 5), (4, 3, 8), (5, 3, 64), (6, 4, 32), (33, 7, 257), (16, 5, 24), (64, 10, 256),
              (130, 3, 48), (64, 40, 64)]
    out = []
    for i, (N, M, C) in enumerate(shapes):
        e = ref.embeddings(N, M, C, seed=100 + i, normalise=i % 3 != 2, spread=0.3)
        p, _, _ = ref.similarity_matrix(e)
        out.append((f"{N}x{M}x{C}", ref.labels(N, M).reshape(-1), p.reshape(-1)))
    y, s = out[4][1], out[4][2]
    out.append(("quantised", y, np.round(s * 2.0) / 2.0))          # many ties
    out.append(("coarse", out[7][1], np.round(out[7][2])))
    out.append(("separable", np.array([1, 1, 1, 0, 0]), np.array([0.9, 0.8, 0.7, 0.3, 0.1])))
    out.append(("inverted", np.array([0, 0, 1, 1, 1]), np.array([0.9, 0.8, 0.7, 0.3, 0.1])))
    out.append(("tied", np.array([0, 1, 1, 0, 1]), np.full(5, 0.25)))
    return out


def test_eer_edge_values_are_exact():
    sets = {n: (y, s) for n, y, s in _score_sets()}
    assert equal_error_rate(*sets["separable"]) == 0.0
    assert equal_error_rate(*sets["inverted"]) == 1.0
    assert equal_error_rate(*sets["tied"]) == 0.5
    # a vertical segment: the curve jumps over tpr = 1 - fpr at fpr = 0.5
    assert equal_error_rate([0, 1, 1, 0], [4, 3, 2, 1]) == 0.5
    # shapes other than flat, and labels as booleans
    assert equal_error_rate(np.array([[True, False], [False, True]]), np.array([[2.0, 1.0], [0.5, 3.0]])) == 0.0
    for bad in (([1, 1], [0.1, 0.2]), ([0, 0], [0.1, 0.2]), ([0, 1], [0.1, float("nan")]), ([0, 2], [0.1, 0.2]),
                ([0, 1, 1], [0.1, 0.2])):
        with pytest.raises(ValueError):
            equal_error_rate(*bad)


def test_eer_vs_sklearn_scipy_pipeline():
    pytest.importorskip("sklearn")
    pytest.importorskip("scipy")
    from scipy.interpolate import interp1d
    from scipy.optimize import brentq
    from sklearn.metrics import roc_curve
    for name, y, s in _score_sets():
        fpr, tpr, _ = roc_curve(y, s)
        want = brentq(lambda x: 1. - x - interp1d(fpr, tpr)(x), 0., 1.)   # lstm_speaker_encoder.py:144-145
        got = equal_error_rate(y, s)
        print(f"EER {name}: {got:.12f} (pipeline {want:.12f}, diff {abs(got - want):.2e})")
        assert abs(got - want) < 1e-9, name


# ---------------------------------------------------------------------------------------------------------- bounds
BOUND_CASES = [((4, 3, 8), True, 10.0, -5.0), ((6, 4, 32), True, 10.0, -5.0), ((5, 3, 16), False, 7.5, -2.0),
               ((33, 7, 257), True, 10.0, -5.0)]


def _fp32_chain(e, w, b):
    """The formulas in numpy float32 (numpy's own summation orders): an implementation the bounds must ACCEPT."""
    e = np.asarray(e, np.float32)
    N, M, C = e.shape
    f = np.float32
    S = e.sum(axis=1, dtype=np.float32)
    c = S / f(M)
    c_hat = c / np.sqrt((c * c).sum(axis=1, keepdims=True, dtype=np.float32))
    x = (S[:, None, :] - e) / f(M - 1)
    x_hat = x / np.sqrt((x * x).sum(axis=2, keepdims=True, dtype=np.float32))
    rows = e.reshape(N * M, C)
    p1 = rows @ c_hat.T
    p2 = (rows * x_hat.reshape(N * M, C)).sum(axis=1, dtype=np.float32)
    s = p1.copy()
    s[np.arange(N * M), ref.own_speaker(N, M)] = p2
    p = s * f(w) + f(b)
    assert p.dtype == np.float32
    t = ref.row_terms(p.astype(np.float64), M)
    return {"p": p, "p1": p1.reshape(-1), "p2": p2, "terms": t, "loss": float(t.mean())}


@pytest.mark.parametrize("shape,unit,w,b", BOUND_CASES)
def test_bounds_accept_a_float32_evaluation(shape, unit, w, b):
    e = ref.embeddings(*shape, seed=7, normalise=unit)
    want, bd, got = ref.loss(e, w, b), gb.bounds(e, w, b), _fp32_chain(e, w, b)
    rs = {k: ratio(got[k], want[k], bd[k]) for k in ("p", "p1", "p2", "terms", "loss")}
    print(f"float32 numpy chain {shape}: " + ", ".join(f"{k} {v:.4f}" for k, v in rs.items()))
    assert max(rs.values()) <= 1.0, rs


@pytest.mark.parametrize("shape,unit,w,b", BOUND_CASES)
def test_bounds_reject_the_mutants(shape, unit, w, b):
    e = ref.embeddings(*shape, seed=7, normalise=unit)
    want, bd = ref.loss(e, w, b), gb.bounds(e, w, b)
    caught_by = {"incl_diag": ("p", "terms", "loss"), "excl_nosub": ("p2", "p", "terms", "loss"), "no_wb": ("p", "terms", "loss"),
                 "target_shift": ("terms", "loss")}
    assert set(caught_by) == set(ref.MUTANTS)
    for m, keys in caught_by.items():
        wrong = ref.loss(e, w, b, mutant=m)
        for k in keys:
            r = ratio(wrong[k], want[k], bd[k])
            assert r > 1.0, f"{m} passes the bound on {k} (ratio {r:.3f})"


def test_bounds_are_small_against_the_values():
    """A bound that admits a relative error of 1e-3 of a unit-scale similarity would check nothing."""
    e = ref.embeddings(64, 10, 256, seed=8)
    bd = gb.bounds(e, 10.0, -5.0)
    assert bd["p1"].max() < 1e-4 and bd["p2"].max() < 1e-4 and bd["p"].max() < 1e-3 and bd["loss_f32"] < 2e-3


def test_shape_error_is_a_value_error():
    assert issubclass(GE2EShapeError, ValueError) and issubclass(GE2EShapeError, NotImplementedError)
