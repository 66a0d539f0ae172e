"""The fp64 restatement of the multi-resolution STFT loss (tests/stft_loss_ref.py) and its derived bound, without a GPU:
the restatement reproduces the reference's own output (tests/golden/stft_loss.npz, fp32 over an FFT), the bound accepts a
float32 evaluation of the dense-DFT path and rejects four subtly wrong ones.  ``SWEEP-RATIO`` lines give error / bound."""
import functools
import os

import numpy as np
import pytest

import fp32_bounds as fb
import stft_loss_cases as lc
import stft_loss_ref as lr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(GOLD, "stft_loss.npz")))


@functools.lru_cache(maxsize=None)
def _case(r):
    """-> xs, ys, [(sums, bound, Field x, Field y) per pair]"""
    xs, ys = lc.batch(r)
    return xs, ys, [lr.sums_with_bound(x, y, r) for x, y in zip(xs, ys)]


def _golden_sums(r):
    g = _gold()
    per = [lr.sums_with_bound(x, y, r) for x, y in zip(g["x"], g["y"])]
    s, bs = sum(p[0] for p in per), sum(p[1] for p in per)
    return per, s, bs, sum(p[2].X.size for p in per)


def test_cases_are_what_they_claim():
    for r in lc.RESOLUTIONS:
        lens = lc.lengths(r)
        assert lens[0] == r.n_fft // 2 + 1 and 4800 < lens[2] < 5000
        F = sum(lc.num_frames(r, n) for n in lens)
        for rows in (F, 2 * F):
            assert rows % 4 != 0 and rows % lc.GEMM_BM != 0, (r, rows)
        xs, ys = lc.batch(r)
        assert not xs[1].any() and all(len(x) == len(y) for x, y in zip(xs, ys))
        assert lr.frames(xs[0], r).shape == (lc.num_frames(r, lens[0]), r.n_fft)
    assert sorted(r.hop % 4 for r in lc.RESOLUTIONS[:4]) == [0, 1, 2, 3]
    assert (lc.RESOLUTIONS[3].n_fft - lc.RESOLUTIONS[3].win) // 2 == 17


@pytest.mark.parametrize("r", lc.RESOLUTIONS, ids=lc.res_id)
def test_restatement_reproduces_the_reference(r):
    """The golden is fp32 over an FFT (and a float64 window); the restatement is fp64: magnitudes and the two losses agree
    under the case's own derived bound."""
    g = _gold()
    per, s, bs, entries = _golden_sums(r)
    for b in range(len(per)):
        q = fb.ratio(g["mag_x_" + lc.res_id(r)][b], per[b][2].X, per[b][2].b_X)
        print(f"SWEEP-RATIO stft_loss golden magnitude {lc.res_id(r)} b={b} {q:.4f}")
        assert q <= 1.0
    sc, mag, b_sc, b_mag = lr.loss_bounds(s, bs, entries)
    want = g["stft_loss"][lc.RESOLUTIONS.index(r)]
    q = max(abs(want[0] - sc) / b_sc, abs(want[1] - mag) / b_mag)
    print(f"SWEEP-RATIO stft_loss golden losses {lc.res_id(r)} {q:.4f} sc={sc:.6f} mag={mag:.6f}")
    assert q <= 1.0
    # the plain functions say the same as the sums
    x_mag, y_mag = lr.stft(g["x"], r), lr.stft(g["y"], r)
    assert np.isclose(lr.spectral_convergence(x_mag, y_mag), sc, rtol=1e-12)
    assert np.isclose(lr.log_stft_magnitude(x_mag, y_mag), mag, rtol=1e-12)


def test_restatement_reproduces_the_multi_resolution_loss():
    g = _gold()
    parts = [lr.loss_bounds(*_golden_sums(r)[1:]) for r in lc.RECIPE]
    sc, mag = np.mean([p[0] for p in parts]), np.mean([p[1] for p in parts])
    b_sc, b_mag = np.mean([p[2] for p in parts]), np.mean([p[3] for p in parts])
    for key in ("multi_resolution", "multi_resolution_bct"):
        q = max(abs(g[key][0] - sc) / b_sc, abs(g[key][1] - mag) / b_mag)
        print(f"SWEEP-RATIO stft_loss golden {key} {q:.4f}")
        assert q <= 1.0
    got = lr.multi_resolution(g["x"], g["y"], lc.RECIPE)
    assert np.allclose(got, (sc, mag), rtol=1e-12)
    assert np.allclose(lr.multi_resolution(g["x"][None], g["y"][None], lc.RECIPE), (sc, mag), rtol=1e-12)


@pytest.mark.parametrize("r", lc.RESOLUTIONS, ids=lc.res_id)
def test_bound_accepts_float32_dense_dft(r):
    xs, ys, per = _case(r)
    for b, (x, y) in enumerate(zip(xs, ys)):
        s, bs, fx, fy = per[b]
        X, Y = lr.dense_f32(x, r), lr.dense_f32(y, r)
        qm = max(fb.ratio(X, fx.X, fx.b_X), fb.ratio(Y, fy.X, fy.b_X))
        qs = fb.ratio(lr.sums_f32(X, Y), s, bs)
        print(f"SWEEP-RATIO stft_loss float32 {lc.res_id(r)} b={b} magnitude {qm:.4f} sums {qs:.4f}")
        assert qm <= 1.0 and qs <= 1.0


@pytest.mark.parametrize("r", lc.RESOLUTIONS, ids=lc.res_id)
def test_bound_rejects_mutants(r):
    """A dropped last frame, a dropped Nyquist bin, frames that start one sample late and a floor of 1e-10 on the silent
    signal each leave the bound of at least one pair: that of its three sums or, where the wrong evaluation keeps the shape
    of the magnitudes, that of an entry of them (the GPU tests hold the engine against both)."""
    xs, ys, per = _case(r)
    worst = {}
    for b, (x, y) in enumerate(zip(xs, ys)):
        s, bs, fx, fy = per[b]
        for name, (m, mags) in lr.mutants(x, y, r, silent_x=not x.any()).items():
            q = fb.ratio(m, s, bs)
            if mags is not None:
                q = max(q, fb.ratio(mags[0], fx.X, fx.b_X), fb.ratio(mags[1], fy.X, fy.b_X))
            worst[name] = max(worst.get(name, 0.0), q)
    print(f"SWEEP-RATIO stft_loss mutants {lc.res_id(r)} " + " ".join(f"{k}={v:.1f}" for k, v in worst.items()))
    assert set(worst) == {"last_frame", "nyquist", "off_by_one", "floor"}
    for name, q in worst.items():
        assert q > 1.0, (name, q)


def test_scaling_case_is_clear_of_the_floor():
    """The scaling test of the GPU suite needs every entry above the floor at 2^-20 times the loud batch."""
    r = lc.RESOLUTIONS[4]
    for v in sum(lc.loud_batch(r), []):
        f = lr.Field(v.astype(np.float64) * 2.0 ** -20, r)
        assert ((f.X - f.b_X) ** 2 > 4.0 * lr.POWER_FLOOR).all()
