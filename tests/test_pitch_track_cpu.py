"""Viterbi tracking over the pitch estimator's candidates, without a device: the restatement (tests/pitch_track_ref.py) against
a brute-force search over every state sequence, what it does where the frame-by-frame picker of tests/pitch_ref.py jumps an
octave (the "hard signal"), that it loses nothing on the estimator's own test signal, and the arguments of ``audio.Pitch``.

Synthetic signals only: nobody has run either estimator on recorded speech."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pitch_ref as pr  # noqa: E402
import pitch_track_ref as ptr  # noqa: E402

RECIPES = [(24000, 300), (22050, 256)]
_HARD, _STD = {}, {}


def _problem(rng, nf, K, dyadic):
    """Random tiny problem: per frame 0 ... K candidates at distinct ascending lags 2 ... 9, an arbitrary table T.  ``dyadic``:
    every number is a small multiple of 1 / 8, so sums are exact and equal path costs are common."""
    lag = np.zeros((nf, K), np.int64)
    cost = np.full((nf, K), np.inf)
    for i in range(nf):
        n = int(rng.integers(0, K + 1))
        lag[i, :n] = np.sort(rng.choice(np.arange(2, 10), n, replace=False))
        cost[i, :n] = rng.integers(0, 5, n) / 8.0 if dyadic else rng.uniform(0, 0.5, n)
    T = np.concatenate([[0.0], rng.integers(0, 4, 9) / 4.0]) if dyadic else ptr.log_tau(9)
    lam, cu, sw = (float(rng.integers(0, 3)) / 2, float(rng.integers(0, 4)) / 8, float(rng.integers(0, 3)) / 8) if dyadic else \
        tuple(rng.uniform(0, 1, 3) * (1.0, 0.3, 0.2))
    return lag, cost, T, lam, cu, sw


@pytest.mark.parametrize("dyadic", [True, False])
def test_restatement_equals_brute_force(dyadic):
    rng = np.random.default_rng(11 + dyadic)
    ties = 0
    for _ in range(150):
        nf, K = int(rng.integers(1, 7)), int(rng.integers(1, 4))
        lag, cost, T, lam, cu, sw = _problem(rng, nf, K, dyadic)
        states, lagv, score = ptr.viterbi(lag, cost, T, lam, cu, sw)
        want, want_score, n_opt = ptr.brute_force(lag, cost, T, lam, cu, sw)
        assert score == want_score
        assert np.array_equal(states, want), (lag, cost, T, lam, cu, sw)
        assert np.array_equal(lagv, [lag[i, s] if s < K else 0 for i, s in enumerate(want)])
        ties += n_opt > 1
    if dyadic:
        print(f"problems with more than one optimal sequence: {ties} of 150")
        assert ties >= 30


def test_engineered_ties():
    T = ptr.log_tau(16)
    inf = np.inf
    # two frames, two candidates an octave apart with equal costs: every voiced path costs the same; smallest last state, then
    # the smallest predecessor
    lag = np.array([[4, 8], [4, 8]])
    cost = np.array([[0.25, 0.25], [0.25, 0.25]])
    states, lagv, score = ptr.viterbi(lag, cost, T, 0.0, 1.0, 0.5)
    assert list(states) == [0, 0] and score == 0.5
    assert list(ptr.brute_force(lag, cost, T, 0.0, 1.0, 0.5)[0]) == [0, 0]
    # the unvoiced state ties with a voiced one: voiced (the smaller state) wins at the end and as a predecessor
    states, _, score = ptr.viterbi(lag, cost, T, 0.0, 0.25, 0.0)
    assert list(states) == [0, 0] and score == 0.5
    # a frame without candidates forces unvoiced; sw = 0 and cu = 0
    lag = np.array([[4, 0], [0, 0], [8, 0]])
    cost = np.array([[0.125, inf], [inf, inf], [0.125, inf]])
    states, lagv, score = ptr.viterbi(lag, cost, T, 1.0, 0.0, 0.0)
    assert list(states) == [2, 2, 2] and list(lagv) == [0, 0, 0] and score == 0.0
    states, lagv, score = ptr.viterbi(lag, cost, T, 1.0, 0.5, 0.0)
    assert list(states) == [0, 2, 0] and list(lagv) == [4, 0, 8] and score == 0.75
    assert list(ptr.brute_force(lag, cost, T, 1.0, 0.5, 0.0)[0]) == [0, 2, 0]


def test_candidates():
    tau_min, tau_max = 3, 12
    r = np.ones((1, tau_max + 1), np.float32)
    r[0, [3, 5, 6, 8, 11]] = [0.2, 0.1, 0.1, 0.2, 0.05]               # 3 = tau_min, 5-6 a plateau (<=: 5 is the minimum), 11 = tau_max - 1
    lag, cost = ptr.candidates(r, tau_min, tau_max, 0.5, 8)
    assert list(lag[0]) == [3, 5, 8, 11, 0, 0, 0, 0] and cost.dtype == np.float32
    assert np.array_equal(cost[0, :4], np.float32([0.2, 0.1, 0.2, 0.05])) and np.all(cost[0, 4:] == np.inf)
    lag, _ = ptr.candidates(r, tau_min, tau_max, 0.5, 3)              # the 3 smallest by (d', tau): 11, 5, then 3 before 8
    assert list(lag[0]) == [3, 5, 11]
    lag, _ = ptr.candidates(r, tau_min, tau_max, 0.15, 8)
    assert list(lag[0, :3]) == [5, 11, 0]
    r[0, 2] = 0.0                                                    # below tau_min: never a candidate, and 3 no longer a minimum
    assert list(ptr.candidates(r, tau_min, tau_max, 0.5, 8)[0][0, :3]) == [5, 8, 11]


def _hard(sr, hop, seed):
    key = (sr, hop, seed)
    if key not in _HARD:
        x = ptr.hard_signal(sr, seed)
        tau_min, tau_max = pr.lags(sr, 80, 400)
        _HARD[key] = (x, pr.cmnd(x, hop, tau_max))
    return _HARD[key]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("sr,hop", RECIPES)
def test_hard_signal_picker_jumps_tracker_does_not(sr, hop, seed):
    tau_min, tau_max = pr.lags(sr, 80, 400)
    eps = pr.eps_d(2 * tau_max, tau_max)
    x, dp64 = _hard(sr, hop, seed)
    for name, dp in (("fp64", dp64), ("fp32", dp64.astype(np.float32))):
        res = pr.pick(dp, sr, tau_min, tau_max)
        gross, _ = ptr.gross_errors(res["f0"], sr, hop)
        decided = pr.decided(res, eps)[gross]
        tr = ptr.track(dp, sr, tau_min, tau_max)
        t_gross, t_unv = ptr.gross_errors(tr["f0"], sr, hop)
        ratio = res["f0"][gross] / pr.f0_true(np.arange(gross.size) * hop / sr)[gross]
        print(f"hard {sr}/{hop} seed {seed} {name}: picker {gross.sum()} gross errors ({decided.sum()} decided, f0 / true "
              f"{ratio.min() if gross.any() else 0:.3f} ... {ratio.max() if gross.any() else 0:.3f}); tracker {t_gross.sum()} gross, "
              f"{t_unv.sum()} unvoiced")
        assert gross.sum() >= 3
        assert decided.all()
        assert t_gross.sum() == 0
        assert t_unv.sum() <= 4


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("sr,hop", RECIPES)
def test_tracker_meets_the_estimators_bars_on_its_signal(sr, hop, seed):
    tau_min, tau_max = pr.lags(sr, 80, 400)
    x = pr.make_signal(sr, seed)
    tr = ptr.track(pr.cmnd(x, hop, tau_max), sr, tau_min, tau_max)
    kind, tc, seg = pr.frame_kinds(sr, hop, x.size)
    voiced = tr["lag"] > 0
    in_v = kind == "v"
    err = np.abs(tr["f0"][voiced & in_v] / pr.f0_true(tc[voiced & in_v]) - 1.0)
    share = (voiced & in_v).sum() / in_v.sum()
    per_silent = [int((voiced & (seg == s)).sum()) for s in pr.SILENT]
    print(f"{sr}/{hop} seed {seed}: {share:.1%} of the voiced segments' frames voiced, f0 error max {err.max():.4%}; voiced in "
          f"noise {(voiced & (kind == 'n')).sum()}, per silent segment {per_silent}")
    assert err.max() <= 0.01
    assert share >= 0.85
    assert not (voiced & (kind == "n")).any()
    assert max(per_silent) <= 1


def test_pitch_arguments():
    """The constructor's checks come before anything touches a device."""
    from parakeet_amd.audio import Pitch
    for kw in (dict(tracker="median"), dict(max_candidates=0), dict(max_candidates=9), dict(max_candidates=2.5),
               dict(candidate_threshold=float("nan")), dict(octave_cost=-1.0), dict(switch_cost=float("nan")),
               dict(unvoiced_cost=-0.5), dict(unvoiced_cost=float("inf"))):
        with pytest.raises(ValueError):
            Pitch(24000, 300, 80, 400, **kw)
