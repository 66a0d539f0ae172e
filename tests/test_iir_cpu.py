"""The restatement tests/iir_ref.py of csrc/pk_iir.h against scipy and against ITU-R BS.1770's own
figures, and the argument checks of the Python layer that need no device.

  * the chunk plan against ``scipy.signal.sosfilt`` in float64: <= 1e-10 max|y| on 200 * 256 + 5 samples of noise (the worst
    measured is 5.7e-14 on these seeded inputs, 4.1e-13 over the wider set of rates; the bar leaves more than 200 x and still
    catches any wrong coefficient or carry); pre-emphasis is exact;
  * ``audio.k_weighting(48000)`` within 1e-14 of the Recommendation's table (8.9e-16 measured);
  * the Recommendation's check signal: a full-scale 997 Hz sine at 48 kHz reads -3.01 LKFS within 0.01;
  * the gates, linearity in the level, and the refusals."""
import os
import sys

import numpy as np
import pytest
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import iir_ref as R  # noqa: E402

BS1770_48K = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                       [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])
MARGIN = 1e-6


def _filters():
    bp, ap = signal.iirpeak(100, 30, fs=22050)
    return {"k16000": R.k_weighting(16000), "k22050": R.k_weighting(22050), "k48000": R.k_weighting(48000),
            "deemph": R.lfilter_sos([1.0], [1.0, -0.97]), "peakQ30": R.lfilter_sos(bp, ap),
            "butter8": signal.butter(8, 300, "hp", fs=22050, output="sos")}


def _noise():
    return (0.1 * np.random.default_rng(1).standard_normal(200 * R.CHUNK + 5)).astype(np.float32)


@pytest.mark.parametrize("name", ["k16000", "k22050", "k48000", "deemph", "peakQ30", "butter8"])
def test_chunk_plan_matches_scipy_sosfilt(name):
    sos = _filters()[name]
    x = _noise()
    y = R.sosfilt64(sos, x)
    w = signal.sosfilt(sos, x.astype(np.float64))
    rel = np.abs(y - w).max() / np.abs(w).max()
    print(f"{name}: chunk plan vs scipy.signal.sosfilt, relative to max|y|: {rel:.3g}")
    assert rel <= 1e-10


def test_preemphasis_is_exact():
    sos = R.lfilter_sos([1.0, -0.97], [1.0])
    x = _noise()
    assert (R.sosfilt64(sos, x) == signal.sosfilt(sos, x.astype(np.float64))).all()


def test_transition_matrix_is_a_chunk_of_zero_input():
    sos = _filters()["butter8"]
    P = R.transition(sos)
    n = P.shape[0]
    for j in range(n):
        zi = np.zeros((sos.shape[0], 2))
        zi.reshape(-1)[j] = 1.0
        _, zf = signal.sosfilt(sos, np.zeros(R.CHUNK), zi=zi)
        assert np.abs(P[:, j] - zf.reshape(-1)).max() <= 1e-12 * max(1.0, np.abs(zf).max())


def test_k_weighting_reproduces_the_table_at_48k():
    from parakeet_amd import audio
    k = audio.k_weighting(48000)
    assert k.shape == (2, 6) and k.dtype == np.float64
    d = np.abs(k - BS1770_48K).max()
    print(f"k_weighting(48000) against the BS.1770 table: {d:.3g}")
    assert d <= 1e-14
    for sr in (8000, 16000, 22050, 44100, 192000):
        assert (audio.k_weighting(sr) == R.k_weighting(sr)).all()


def test_997_hz_full_scale_sine_reads_minus_3_01():
    out = {}
    for sr in (48000, 22050, 16000):
        t = np.arange(3 * sr) / sr
        d = R.loudness(np.sin(2 * np.pi * 997 * t).astype(np.float32), sr)
        out[sr] = d
        print(f"997 Hz full scale at {sr} Hz: {d['lufs']:.5f} LUFS, {d['blocks']} blocks, {d['gated']} kept")
    assert abs(out[48000]["lufs"] - (-3.01)) <= 0.01
    assert out[48000]["blocks"] == 27 and out[48000]["gated"] == 27


def _clear_of_thresholds(d):
    """every block power stays clear of both thresholds by a relative MARGIN"""
    p = d["p"]
    for thr in (R.ABS, d["rel"]):
        if thr > 0 and len(p):
            assert (np.abs(p - thr) > MARGIN * thr).all()


def test_gate_drops_the_quiet_half():
    sr = 22050
    t = np.arange(2 * sr) / sr
    loud, quiet = 0.5 * np.sin(2 * np.pi * 440 * t), 0.005 * np.sin(2 * np.pi * 440 * t)
    x = np.concatenate([loud, quiet]).astype(np.float32)
    d = R.loudness(x, sr)
    _clear_of_thresholds(d)
    z = signal.sosfilt(R.k_weighting(sr), x.astype(np.float64))
    ungated = -0.691 + 10 * np.log10(np.mean(z ** 2))
    print(f"loud + quiet: gated {d['lufs']:.3f} LUFS ({d['gated']} of {d['blocks']} blocks), ungated mean square {ungated:.3f}")
    assert d["gated_abs"] == d["blocks"] and 0 < d["gated"] < d["blocks"]
    assert d["lufs"] > ungated + 2.0
    only = R.loudness(loud.astype(np.float32), sr)
    assert only["lufs"] - 0.5 < d["lufs"] < only["lufs"]       # the blocks that straddle the step survive the gate
    # the relative gate, computed another way: -10 LU below the mean of the blocks above the absolute gate
    p = d["p"]
    want_rel = 0.1 * p[p > R.ABS].mean()
    assert abs(d["rel"] - want_rel) <= 1e-12 * want_rel
    assert d["gated"] == int((p > want_rel).sum())


def test_below_the_absolute_gate_and_too_short_give_minus_infinity():
    sr = 16000
    t = np.arange(2 * sr) / sr
    x = (1e-4 * np.sin(2 * np.pi * 440 * t)).astype(np.float32)           # about -83 LUFS
    d = R.loudness(x, sr)
    _clear_of_thresholds(d)
    assert d["blocks"] == 17 and d["gated_abs"] == 0 and d["gated"] == 0 and d["lufs"] == -np.inf and d["mean_power"] == 0.0
    short = (0.5 * np.sin(2 * np.pi * 440 * np.arange(4 * 1600 - 1) / sr)).astype(np.float32)     # one sample short of 400 ms
    d = R.loudness(short, sr)
    assert d["blocks"] == 0 and d["lufs"] == -np.inf
    d = R.loudness(np.zeros(0, np.float32), sr)
    assert d["blocks"] == 0 and d["lufs"] == -np.inf and d["peak"] == 0


def test_doubling_the_level_adds_20_log10_2():
    sr = 22050
    x = (0.05 * np.random.default_rng(3).standard_normal(2 * sr)).astype(np.float32)
    a, b = R.loudness(x, sr), R.loudness((2 * x).astype(np.float32), sr)       # doubling a float32 is exact
    _clear_of_thresholds(a)
    _clear_of_thresholds(b)
    assert a["gated"] == b["gated"] > 0
    assert abs((b["lufs"] - a["lufs"]) - 20 * np.log10(2.0)) <= 1e-9


def test_segments_are_the_sums_of_squares():
    sr = 8000
    z = np.random.default_rng(5).standard_normal(5 * 800 + 123)
    seg = R.segments(z, sr)
    want = (z[:5 * 800] ** 2).reshape(5, 800).sum(1)
    assert seg.shape == (5,) and np.abs(seg - want).max() <= 1e-12 * want.max()


def test_argument_errors_need_no_device():
    from parakeet_amd import audio, metrics
    x = np.zeros(1000, np.float32)
    with pytest.raises(ValueError):
        audio.sosfilt([[1.0, 0.0, 0.0, 2.0, 0.0, 0.0]], x)                     # a0 != 1
    with pytest.raises(ValueError):
        audio.sosfilt([[1.0, 0.0, 0.0, 1.0, np.nan, 0.0]], x)
    with pytest.raises(ValueError):
        audio.sosfilt(np.zeros((0, 6)), x)                                      # no section
    with pytest.raises(ValueError):
        audio.sosfilt(np.zeros((2, 5)), x)
    with pytest.raises(NotImplementedError):
        audio.sosfilt(signal.butter(18, 0.2, output="sos"), x)                  # 9 sections
    with pytest.raises(NotImplementedError, match="sosfilt"):
        audio.lfilter([1.0, 0.5, 0.25, 0.125], [1.0], x)
    with pytest.raises(NotImplementedError, match="sosfilt"):
        audio.lfilter([1.0], [1.0, 0.5, 0.25, 0.125], x)
    with pytest.raises(ValueError):
        audio.lfilter([1.0], [0.0, 1.0], x)
    for sr in (22051, 4000, 200000):
        with pytest.raises(NotImplementedError):
            audio.k_weighting(sr)
        with pytest.raises(NotImplementedError):
            metrics.loudness_batch([x], sr)
        with pytest.raises(NotImplementedError):
            audio.normalize_loudness_batch([x], sr)
    with pytest.raises(ValueError):
        audio.k_weighting(-16000)
    with pytest.raises(ValueError):
        audio.normalize_loudness_batch([x], 16000, target_lufs=float("nan"))
    with pytest.raises(ValueError):
        audio.normalize_loudness_batch([x], 16000, max_peak=0.0)
    with pytest.raises(ValueError):
        metrics.loudness(list(x), 16000)
    assert (audio._lfilter_sos([2.0, 1.0], [2.0, -1.0]) == [[1.0, 0.5, 0.0, 1.0, -0.5, 0.0]]).all()


def test_every_new_export_is_bound():
    from parakeet_amd import _capi
    bound = _capi._declare(_capi.lib())
    for name in ("pk_iir_create", "pk_iir_destroy", "pk_iir_transition", "pk_iir_run", "pk_loudness_run", "pk_gain_run"):
        assert name in bound
    header = open(os.path.join(os.path.dirname(HERE), "include", "pk_synth.h")).read()
    for name in ("pk_iir_create", "pk_loudness_run", "pk_gain_run"):
        assert name + "(" in header


def test_the_header_and_the_restatement_share_their_constants():
    src = open(os.path.join(os.path.dirname(HERE), "parakeet_amd", "csrc", "pk_iir.h")).read()
    assert "IIR_CHUNK = 256" in src and f"LOUD_ABS = {R.ABS!r}" in src and "LOUD_THREADS = 256" in src
    from parakeet_amd import audio
    assert (audio.IIR_CHUNK, audio.IIR_MAX_SECTIONS) == (R.CHUNK, R.MAX_SECTIONS)
    assert (audio.LOUDNESS_SR_MIN, audio.LOUDNESS_SR_MAX) == (R.SR_MIN, R.SR_MAX)
