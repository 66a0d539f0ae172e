"""The restatement tests/pvoc_ref.py of csrc/pk_pvoc.h against the literal formula of librosa 0.8's
``phase_vocoder`` (angle, wrap, cumulative sum in float64, written out in pvoc_ref.literal_phase_vocoder), and the checks of
the Python layer that need no device.

  * phasor form against literal formula, both BEFORE the float32 rounding: at most (pi hop T^2 + 16 T) 2^-52 max|D|.  The
    first term is the literal formula's own accumulated rounding of a phase of size pi hop T over T additions, the second a
    few ulp per phasor step.  Measured on these seeded inputs (max|D| = 9.1): n_fft 64 / hop 16, 177 frames: 1.3e-10 at rate
    0.5 (T = 354, bound 1.3e-8), 3.7e-11 at 0.7, 2.2e-11 at 1.0, 1.6e-11 at 1.3, 9.3e-12 at 2.0, 2.2e-12 at 3.7 (T = 48, bound
    2.4e-10); n_fft 128 / hop 32, 126 frames: 1.6e-10 at rate 0.5 (T = 252, bound 1.3e-8) down to 4.4e-12 at 3.7;
  * T against ``len(numpy.arange(0, F, rate))``, the edge cases, rate 1.0, the pitch ratios, the refusals, the exports."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pvoc_ref as R  # noqa: E402

RATES = (0.5, 0.7, 1.0, 1.3, 2.0, 3.7)


def _spectrum(n_fft, F, seed=0):
    rng = np.random.default_rng(seed)
    nb = n_fft // 2 + 1
    return (2.0 * (rng.standard_normal((nb, F)) + 1j * rng.standard_normal((nb, F)))).astype(np.complex64)


@pytest.mark.parametrize("n_fft,hop,F", [(64, 16, 177), (128, 32, 126)])
@pytest.mark.parametrize("rate", RATES)
def test_phasor_form_matches_the_literal_formula(n_fft, hop, F, rate):
    D = _spectrum(n_fft, F)
    got = R.from_rows(R.phase_vocoder_rows64(R.to_rows(D), rate))
    want = R.literal_phase_vocoder(D, rate, hop)
    assert got.shape == want.shape
    T = got.shape[1]
    dmax = float(np.abs(D).max())
    bound = (math.pi * hop * T ** 2 + 16 * T) * 2.0 ** -52 * dmax
    err = float(np.abs(got - want).max())
    print(f"n_fft {n_fft} hop {hop} rate {rate}: T = {T}, max|D| = {dmax:.3g}, phasor form vs literal formula {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_hop_length_has_no_effect_on_the_literal_formula_beyond_its_rounding():
    D = _spectrum(64, 40, seed=1)
    a, b = R.literal_phase_vocoder(D, 0.7, 16), R.literal_phase_vocoder(D, 0.7, 64)
    T = a.shape[1]
    assert np.abs(a - b).max() <= 2 * (math.pi * 64 * T ** 2 + 16 * T) * 2.0 ** -52 * np.abs(D).max()


def test_frame_count_is_the_length_of_arange():
    from parakeet_amd import audio
    for rate in RATES + (1.0594630943592953, 41.0, 1e-3):
        for F in range(1, 41):
            want = len(np.arange(0, F, rate))
            assert R.num_frames(F, rate) == want, (F, rate)
            assert audio.pvoc_num_frames(F, rate) == want, (F, rate)
            if rate >= 0.5 and F % 7 == 1:
                assert R.phase_vocoder_rows(np.ones((F, 2), np.float32), rate).shape == (want, 2)


def test_zeros_a_single_frame_and_a_rate_beyond_the_frames():
    z = R.phase_vocoder_rows(np.zeros((7, 10), np.float32), 0.7)
    assert z.shape == (10, 10) and (z == 0).all() and not np.signbit(z).any()
    one = R.to_rows(_spectrum(16, 1, seed=2))
    out = R.phase_vocoder_rows(one, 0.4)                       # steps 0, 0.4, 0.8: magnitudes (1 - a) |D[0]|; every step
    assert out.shape == (3, one.shape[1])                      # turns the phase back by angle(D[0]) (D[1] is a zero column,
    nb = one.shape[1] // 2                                     # angle 0): the phases are those of D[0], 1, conj(D[0])
    assert nb == 9
    z = one[0, :nb].astype(np.float64) + 1j * one[0, nb:].astype(np.float64)
    for t, want in enumerate((z, 0.6 * np.abs(z), 0.2 * np.conj(z))):
        got = out[t, :nb].astype(np.float64) + 1j * out[t, nb:].astype(np.float64)
        assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(z).max()
    D = R.to_rows(_spectrum(16, 5, seed=3))
    out = R.phase_vocoder_rows(D, 7.5)
    assert R.num_frames(5, 7.5) == 1 and out.shape == (1, D.shape[1])
    assert np.abs(out[0] - D[0]).max() <= 4 * 2.0 ** -24 * np.abs(D[0]).max()


def test_zero_bins_take_the_unit_phasor():
    D = _spectrum(16, 6, seed=4)
    D[3, :] = 0
    D[5, 2] = 0
    D[:, 4] = 0
    out = R.phase_vocoder(D, 1.0)
    assert (out[3] == 0).all() and out[5, 2] == 0 and (out[:, 4] == 0).all()
    assert np.isfinite(out).all()


def test_rate_one_returns_the_spectrogram():
    D = _spectrum(64, 50, seed=5)
    rows = R.to_rows(D)
    out = R.phase_vocoder_rows(rows, 1.0)
    assert out.shape == rows.shape
    nb = rows.shape[1] // 2
    mod = np.abs(D.T.astype(np.complex128))                    # |D| per (frame, bin)
    err = np.abs(out.astype(np.float64) - rows.astype(np.float64))
    worst = float((np.concatenate([err[:, :nb] / mod, err[:, nb:] / mod])).max())
    print(f"rate 1.0: worst error per component {worst / 2.0 ** -24:.3g} x 2^-24 |D|")
    assert (err[:, :nb] <= 4 * 2.0 ** -24 * mod).all() and (err[:, nb:] <= 4 * 2.0 ** -24 * mod).all()


def test_pitch_shift_ratio():
    from parakeet_amd import audio
    assert audio.pitch_shift_ratio(12) == (Fraction(1, 2), 0.0)
    assert audio.pitch_shift_ratio(-12) == (Fraction(2, 1), 0.0)
    assert audio.pitch_shift_ratio(0) == (Fraction(1, 1), 0.0)
    assert audio.pitch_shift_ratio(24, 24) == (Fraction(1, 2), 0.0)
    worst = 0.0
    for bpo in (12, 24):
        for n in range(-2 * bpo, 2 * bpo + 1):
            fr, cents = audio.pitch_shift_ratio(n, bpo)
            want = 2.0 ** (-n / bpo)
            assert fr == Fraction(want).limit_denominator(1000) and fr.denominator <= 1000
            assert abs(cents) <= 0.03 and abs(1200.0 * math.log2(want / float(fr)) - cents) <= 1e-9
            assert max(fr.numerator, fr.denominator) <= 4096
            worst = max(worst, abs(cents))
    print(f"pitch_shift_ratio: worst over +-2 octaves at 12 and 24 bins per octave {worst:.4f} cent")
    fr, cents = audio.pitch_shift_ratio(7)
    assert abs(float(fr) - 2.0 ** (-7 / 12)) < 1e-6


def test_stretched_length_rounds_ties_to_even():
    from parakeet_amd import audio
    assert audio.stretched_length(5, 2.0) == 2 and audio.stretched_length(7, 2.0) == 4      # 2.5 -> 2, 3.5 -> 4
    assert audio.stretched_length(4000, 0.8) == 5000 and audio.stretched_length(4000, 1.25) == 3200


def test_argument_errors_need_no_device():
    from parakeet_amd import audio
    rows = np.zeros((5, 18), np.float32)
    x = np.zeros(1000, np.float32)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "fast", None):
        with pytest.raises(ValueError):
            audio.phase_vocoder_batch([rows], [bad])
        with pytest.raises(ValueError):
            audio.phase_vocoder(np.zeros((9, 5), np.complex64), bad)
        with pytest.raises(ValueError):
            audio.time_stretch(x, bad)
        with pytest.raises(ValueError):
            audio.time_stretch_batch([x, x], [1.0, bad])
    with pytest.raises(ValueError):
        audio.phase_vocoder_batch([], [])
    with pytest.raises(ValueError):
        audio.phase_vocoder_batch([rows], [1.0, 2.0])                       # one rate per utterance
    with pytest.raises(ValueError):
        audio.phase_vocoder_batch([np.zeros((5, 17), np.float32)], [1.0])   # an odd number of columns
    with pytest.raises(ValueError):
        audio.phase_vocoder_batch([np.zeros((0, 18), np.float32)], [1.0])   # no frame
    with pytest.raises(ValueError):
        audio.phase_vocoder_batch([rows, np.zeros((5, 34), np.float32)], [1.0, 1.0])
    with pytest.raises(ValueError):
        audio.phase_vocoder_batch([np.zeros(18, np.float32)], [1.0])
    with pytest.raises(ValueError):
        audio.phase_vocoder_batch([rows], [1e-9])                           # T = 5e9 >= 2^31
    with pytest.raises(ValueError):
        audio.phase_vocoder(np.zeros((9, 5), np.float32), 1.0)              # not complex
    with pytest.raises(ValueError):
        audio.phase_vocoder(np.zeros((9, 0), np.complex64), 1.0)
    with pytest.raises(ValueError):
        audio.pvoc_num_frames(0, 1.0)
    with pytest.raises(ValueError):
        audio.pvoc_num_frames(2 ** 31 - 1, 0.5)
    with pytest.raises(ValueError):
        audio.time_stretch(np.zeros(0, np.float32), 1.0)                    # empty
    with pytest.raises(ValueError):
        audio.time_stretch(np.zeros((2, 500), np.float32), 1.0)
    with pytest.raises(ValueError):
        audio.time_stretch_batch([], [])
    with pytest.raises(ValueError):
        audio.time_stretch(list(x), 1.0)
    with pytest.raises(ValueError):
        audio.time_stretch(x, 1.0, transform="radix")
    with pytest.raises(ValueError):
        audio.pitch_shift(np.zeros(0, np.float32), 8000, 2)
    for sr in (0, -8000, float("nan"), "8k"):
        with pytest.raises(ValueError):
            audio.pitch_shift(x, sr, 2)
    for steps in (float("nan"), float("inf"), "up"):
        with pytest.raises(ValueError):
            audio.pitch_shift(x, 8000, steps)
    for bpo in (0, -12, 12.5):
        with pytest.raises(ValueError):
            audio.pitch_shift(x, 8000, 2, bins_per_octave=bpo)
    with pytest.raises(ValueError):
        audio.pitch_shift(x, 8000, 1e6)                                     # 2 ** (-1e6 / 12) underflows to 0
    fr, _ = audio.pitch_shift_ratio(-30)                                    # 2 ** 2.5 = 5.657: beyond Resample's terms of 4096
    assert max(fr.numerator, fr.denominator) > audio.RESAMPLE_MAX_RATIO
    with pytest.raises(NotImplementedError, match="envelope"):
        audio.pitch_shift(x, 8000, -30)


def test_every_new_export_is_bound():
    from parakeet_amd import _capi
    bound = _capi._declare(_capi.lib())
    header = open(os.path.join(ROOT, "include", "pk_synth.h")).read()
    for name in ("pk_pvoc_num_frames", "pk_pvoc_run"):
        assert name in bound and name + "(" in header
    from parakeet_amd import build
    assert "pvoc.hip" in build.SOURCES and build.FILE_FLAGS["pvoc.hip"] == build.FILE_FLAGS["iir.hip"]


def test_the_header_and_the_restatement_share_their_constants():
    src = open(os.path.join(ROOT, "parakeet_amd", "csrc", "pk_pvoc.h")).read()
    assert f"PVOC_THREADS = {R.THREADS};" in src and f"PVOC_AHEAD = {R.AHEAD};" in src
    assert f"PVOC_MAX_BATCH = {R.MAX_BATCH};" in src and "PVOC_MAX_FRAMES = (int64_t)1 << 31;" in src and R.MAX_FRAMES == 1 << 31
    from parakeet_amd import audio
    assert audio.PVOC_MAX_FRAMES == R.MAX_FRAMES and audio.PITCH_SHIFT_MAX_DENOMINATOR == 1000
    assert audio.pvoc_num_frames(2 ** 31 - 1, 1.0) == R.MAX_FRAMES - 1
