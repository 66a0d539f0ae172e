"""STOI / ESTOI without a GPU: the float64 restatement tests/stoi_ref.py against the numbers the definition fixes (DESIGN.md
4.7d), the fp32 evaluation of the engine's plan against it, and the host side of the new surface (argument errors, exports)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stoi_ref as sr  # noqa: E402

LO = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
HI = [9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]


def test_band_table():
    from parakeet_amd import metrics
    lo, hi = sr.band_edges()
    assert list(lo) == LO and list(hi) == HI
    elo, ehi = metrics.stoi_band_edges()                     # the engine's table, computed in float64 on the host
    assert list(elo) == LO and list(ehi) == HI
    assert HI[:-1] == LO[1:]                                 # contiguous ranges


def test_frame_rule():
    from parakeet_amd import metrics
    for L, F in ((0, 0), (1, 0), (256, 0), (257, 1), (384, 1), (385, 2), (4096, 30), (4097, 31), (4225, 32), (30000, 233)):
        assert sr.num_frames(L) == F == metrics.stoi_num_frames(L), L
    # K kept frames give (K - 1) 128 + 256 samples and K - 1 spectrum frames
    for K in (1, 2, 3, 31, 257):
        Lr = (K - 1) * 128 + 256
        assert sr.num_frames(Lr) == K - 1
        x = sr.harmonic(257 + 128 * (K - 1), K)
        keep, _ = sr.silent_mask(x)
        assert keep.all() and len(keep) == K and len(sr.rebuild(x, keep)) == Lr
    assert len(sr.rebuild(sr.harmonic(300, 0), np.zeros(1, bool))) == 0


def test_fewer_than_thirty_spectrum_frames_give_nan():
    for ext in (False, True):
        x = sr.harmonic(4096, 0)
        r = sr.stoi(x, sr.add_noise(x, 5, 0), ext)
        assert np.isnan(r["d"]) and (r["segments"], r["kept"], r["frames"]) == (0, 30, 30)
        x = sr.harmonic(4097, 0)
        r = sr.stoi(x, sr.add_noise(x, 5, 0), ext)
        assert np.isfinite(r["d"]) and (r["segments"], r["kept"], r["frames"]) == (1, 31, 31)
        x = sr.harmonic(4225, 0)
        assert sr.stoi(x, x, ext)["segments"] == 2
        assert np.isnan(sr.stoi(np.zeros(100), np.zeros(100), ext)["d"])
        assert np.isnan(sr.stoi_f32(sr.harmonic(4096, 0), sr.harmonic(4096, 0), ext)["d"])


def test_identical_signals_score_one():
    for L in (4097, 9000, 30000):
        x = sr.harmonic(L, L)
        for ext in (False, True):
            assert abs(sr.stoi(x, x, ext)["d"] - 1.0) <= 1e-12
            assert abs(sr.stoi_f32(x, x, ext)["d"] - 1.0) <= 1e-12


def test_scores_fall_with_the_noise():
    x = sr.harmonic(30000, 1)
    for ext in (False, True):
        d = [sr.stoi(x, sr.add_noise(x, snr, 0), ext)["d"] for snr in (30, 10, 0, -10)]
        assert 1.0 > d[0] > d[1] > d[2] > d[3] > 0.0, d
        d32 = [sr.stoi_f32(x, sr.add_noise(x, snr, 0), ext)["d"] for snr in (30, 10, 0, -10)]
        assert np.max(np.abs(np.array(d) - np.array(d32))) < 5e-6          # the plan in fp32 is the same measure


def test_constructed_mask():
    """960 leading zeros and an inner gap of 1 024 exact zeros: the frames that lie wholly inside them are removed, the rest is
    kept (a constant-amplitude signal, so that a frame reaching into the signal by 48 samples is still within 40 dB)."""
    L = 9000
    t = np.arange(L) / sr.FS
    x = (0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 1310.0 * t + 1.0)).astype(np.float32)
    x[:960] = 0.0
    x[4000:5024] = 0.0
    keep, e = sr.silent_mask(x)
    starts = np.arange(len(keep)) * sr.HOP
    inside = (starts + sr.FRAME <= 960) | ((starts >= 4000) & (starts + sr.FRAME <= 5024))
    assert inside.sum() == 6 + 6
    assert np.array_equal(keep, ~inside)
    assert np.all(e[inside] == 20.0 * np.log10(sr.EPS))
    assert sr.threshold_margin(x) >= 0.01
    assert np.array_equal(sr.silent_mask_f32(x), keep)
    r = sr.stoi(x, sr.add_noise(x, 10, 0))
    assert (r["kept"], r["frames"], r["segments"]) == (len(keep) - 12, len(keep), len(keep) - 12 - 30)


def test_all_zero_clean_signal_is_finite():
    z = np.zeros(6000, np.float32)
    for y in (z, sr.harmonic(6000, 0)):
        for ext in (False, True):
            r, r32 = sr.stoi(z, y, ext), sr.stoi_f32(z, y, ext)
            assert np.isfinite(r["d"]) and r["d"] == 0.0 and r == r32
            assert (r["segments"], r["kept"], r["frames"]) == (15, 45, 45)


def test_bounds_are_what_the_derivations_say():
    import fp32_bounds as fb
    import rfft_ref as rr
    assert rr.passes(512) == (4, 0) and abs(rr.rfft_c(512) - (np.sqrt(2.0) * 26 + 8)) < 1e-12
    x = sr.harmonic(4097, 3)
    want = sr.bands(x)
    b = sr.band_bound(x, want)
    assert b.shape == want.shape and np.all(b > 0)
    # the fp32 plan is inside its own bound, and a spectrum scaled by (1 + 2^-10) is not
    got = sr.bands_f32(x).astype(np.float64)
    assert np.max(np.abs(got - want) / b) <= 1.0
    assert np.max(np.abs(want * (1 + 2.0 ** -10) - want) / b) > 1.0
    assert sr.stoi_seg_bound(100.0, 600) == 4 * (26872 + 14 + 11 + 1) * 2.0 ** -53       # 1.2e-11
    assert sr.stoi_seg_bound(100.0, 600) < sr.estoi_seg_bound(100.0, 0.05, 600) < 1e-8
    assert fb.U == 2.0 ** -24


def test_argument_errors():
    from parakeet_amd import _capi, metrics
    x = np.zeros(5000, np.float32)
    with pytest.raises(ValueError, match="one length"):
        metrics.stoi_batch([x], [x[:-1]], 10000)
    with pytest.raises(ValueError, match="2 reference signals, 1 degraded"):
        metrics.stoi_batch([x, x], [x], 10000)
    with pytest.raises(ValueError, match="1-D"):
        metrics.stoi_batch(x.reshape(2, -1), x.reshape(2, -1), 10000)
    with pytest.raises(ValueError, match="no reference signal"):
        metrics.stoi_batch([], [], 10000)
    with pytest.raises(ValueError, match="positive integer"):
        metrics.stoi_batch(x, x, 0)
    with pytest.raises(ValueError, match="lists go to stoi_batch"):
        metrics.stoi([x], [x], 10000)
    with pytest.raises(ValueError, match="one shape"):
        metrics.stoi_from_bands(np.zeros((40, 15), np.float32), np.zeros((41, 15), np.float32))
    with pytest.raises(ValueError, match="one shape"):
        metrics.stoi_from_bands(np.zeros((40, 14), np.float32), np.zeros((40, 14), np.float32))
    lib = _capi.lib()
    offs = (C.c_int64 * 2)(0, 10)
    assert lib.pk_stoi_run(None, None, None, offs, 1, 0, None) == -1 and b"pk_stoi_run" in lib.pk_last_error()
    assert lib.pk_stoi_mask(None, None, offs, 1, None, None, None, None) == -1
    assert lib.pk_stoi_bands(None, None, offs, 1, None) == -1
    assert lib.pk_stoi_segments(None, None, None, None, 1, 0, None, None) == -1
    assert lib.pk_stoi_num_frames(-1, C.byref(C.c_int64())) == -1
    assert lib.pk_stoi_band_edges(None, None) == -1


def test_exports_are_bound():
    from parakeet_amd import _capi, metrics
    bound = _capi._declare(_capi.lib())
    for name in ("pk_stoi_run", "pk_stoi_mask", "pk_stoi_bands", "pk_stoi_segments", "pk_stoi_num_frames", "pk_stoi_band_edges"):
        assert name in bound and hasattr(_capi.lib(), name)
    for name in ("stoi", "stoi_batch", "stoi_silent_frames", "stoi_bands", "stoi_from_bands"):
        assert name in metrics.__all__ and callable(getattr(metrics, name))
    assert C.sizeof(_capi.StoiResult) == 24 == metrics._STOI_RESULT.itemsize
    assert "stoi_batch" not in metrics.score_batch.__code__.co_names      # score_batch stays as it is
