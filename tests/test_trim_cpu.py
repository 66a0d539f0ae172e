"""Silence trimming without a device: the fp64 restatement (tests/trim_ref.py) against the reference's own arithmetic, scipy
and the golden the reference's source wrote; the error bound of the frame power; that the signals the GPU tests use leave no
frame or window undecided (so those tests cannot pass vacuously); the hand-derived result for the released GE2E parameters;
the envelope and the ``vad=None`` path of the GE2E preprocessor."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trim_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vad_post.npz")


def _patterns(n, rng):
    return [rng.uniform(size=n) < p for p in (0.2, 0.5, 0.8)] + [np.repeat(rng.uniform(size=n // 5 + 1) < 0.5, 5)[:n],
                                                                 np.zeros(n, bool), np.ones(n, bool)]


@pytest.mark.parametrize("W", range(1, 12))
def test_smoothing_is_the_references_rounded_moving_average(W):
    rng = np.random.default_rng(W)
    for n in (1, 2, 3, W - 1, W, W + 1, 40, 301):
        for f in _patterns(max(n, 1), rng):
            assert np.array_equal(tr.smooth(f, W), tr.moving_average_rounded(f, W)), (W, n)


@pytest.mark.parametrize("S", range(0, 9))
def test_dilation_is_scipys(S):
    from scipy.ndimage import binary_dilation
    rng = np.random.default_rng(100 + S)
    for n in (1, 2, S, S + 1, S + 2, 40, 301):
        for m in _patterns(max(n, 1), rng):
            assert np.array_equal(tr.dilate(m, S), binary_dilation(m, np.ones(S + 1))), (S, n)


def test_restatement_reproduces_the_references_golden_bit_for_bit():
    cases = tr.vad_golden(GOLDEN)
    assert {c["W"] for c in cases} >= set(range(1, 10)) and {c["S"] for c in cases} >= set(range(0, 9))
    n_w = [c["flags"].size for c in cases]
    assert min(n_w) == 1 and max(n_w) > 300
    assert any(c["wav"].size % tr.window_size(c["ms"], c["sr"]) for c in cases)
    assert any(not c["flags"].any() and c["flags"].size > 1 for c in cases) and any(c["flags"].all() and c["flags"].size > 1 for c in cases)
    for c in cases:
        got = tr.trim_long_silences(c["wav"], c["flags"], tr.window_size(c["ms"], c["sr"]), c["W"], c["S"])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), c["out"].view(np.uint32)), c["name"]


@pytest.mark.parametrize("Lf,hop", [(2048, 512), (1200, 300), (400, 160), (7, 3)])
def test_power_bound_from_the_stated_order(Lf, hop):
    """eps_P counts the roundings of the order csrc/pk_trim.h states; an emulation of that order in float32 stays inside it, and
    it never exceeds the bound that holds for any order."""
    assert tr.eps_P(Lf) <= tr.eps_any_order(Lf)
    rng = np.random.default_rng(Lf)
    x = (rng.standard_normal(4 * Lf + 5 * hop + 3) * np.exp(rng.uniform(-6, 0))).astype(np.float32)
    for mode in ("reflect", "constant"):
        want = tr.frame_power(x, Lf, hop, True, mode)
        got = tr.emulate_power_f32(x, Lf, hop, True, mode)
        assert got.shape == want.shape and want.size == tr.num_frames(x.size, Lf, hop)
        worst = float(np.max(np.abs(got - want) / (tr.eps_P(Lf) * want)))
        print(f"Lf {Lf}: emulated order / eps_P {worst:.4f} (eps_P {tr.eps_P(Lf):.3g})")
        assert worst <= 1.0


def test_reflect_is_numpys_and_needs_more_than_half_a_frame():
    x = np.arange(1, 8, dtype=np.float64)
    P = tr.frame_power(x, 6, 2, True, "reflect")
    pad = np.concatenate([x[3:0:-1], x, x[-2:-5:-1]])
    assert np.allclose(P, [np.mean(pad[i:i + 6] ** 2) for i in range(0, pad.size - 5, 2)], rtol=1e-15)
    with pytest.raises(ValueError):
        tr.frame_power(np.ones(3), 6, 2, True, "reflect")
    assert tr.frame_power(np.ones(1), 6, 2, True, "constant").size == 1
    assert tr.frame_power(np.ones(5), 6, 6, False).size == 0


def test_no_undecided_frame_in_the_signals_the_gpu_tests_use():
    """trim / split / flags on the device are compared with fp64 integers: that is only a test where no frame sits within the
    power's error of the threshold.  Asserted here for every signal those tests use; an input that fails is to be changed."""
    eps = tr.eps_P(2048)
    for name, x in tr.trim_cases().items():
        P = tr.frame_power(x, 2048, 512)
        for top_db in (20, 60):
            und = int((~tr.decided_frames(P, top_db, eps)).sum())
            assert und == 0, (name, top_db, und)
    # what the cases are there for
    c = tr.trim_cases()
    assert tuple(tr.trim_index(c["zeros"])) == (0, 6000)                       # all zeros: every frame non-silent
    a, b = tr.trim_index(c["lead_trail"])
    assert 0 < a < 3333 + 512 and a % 512 == 0 and 3333 % 512 and (3333 + 7001) % 512
    assert tr.trim_index(c["to_last_sample"])[1] == c["to_last_sample"].size and c["to_last_sample"].size % 512   # the clip
    assert tr.split_index(c["bursts"]).shape == (3, 2) and tr.split_index(c["impulse"]).shape == (1, 2)
    for name in ("lead_trail", "bursts", "impulse"):
        assert tr.nonsilent(tr.frame_power(c[name]), 60).sum() < tr.num_frames(c[name].size, 2048, 512)


def test_no_undecided_window_in_the_energy_detector_signals():
    w = tr.window_size(30, 16000)
    for seed in (0, 1):
        x, built = tr.burst_signal(seed=seed)
        Q, flags, thr = tr.energy_flags(x, w)
        assert np.array_equal(flags, built)
        assert tr.decided_windows(Q, thr, tr.eps_P(w)).all()
    x, built = tr.pause_signal()
    Q, flags, thr = tr.energy_flags(x, w)
    assert np.array_equal(flags, built) and tr.decided_windows(Q, thr, tr.eps_P(w)).all()


def test_released_ge2e_parameters_leave_five_windows_of_every_long_silence():
    """(30 ms, 8, 6): the moving average (2 c > 8 over [k - 3, k + 4]) moves a voiced run's end one window in and leaves its
    start, so a silence of G windows is G + 1 in the mask; the dilation (k - 3 ... k + 3) takes three back on either side:
    G - 5 windows are dropped and 5 stay, for every interior G >= 6 between runs of 8 or more."""
    gaps = (6, 7, 9, 14, 25, 60)
    x, flags = tr.burst_signal(gaps=gaps)
    keep = tr.keep_mask(flags, 8, 6)
    dropped = tr.runs(~keep)
    interior = [(a, b) for a, b in dropped if a > 0 and b < keep.size]
    assert [b - a for a, b in interior] == [g - 5 for g in gaps]
    w = tr.window_size(30, 16000)
    out = tr.trim_long_silences(x, flags, w, 8, 6)
    voiced = np.repeat(flags[keep], w)
    silent_runs = tr.runs(~flags[keep])
    assert [b - a for a, b in silent_runs if a > 0 and b < keep.sum()] == [5] * len(gaps)
    assert out.size == keep.sum() * w and voiced.size == out.size


def test_envelope_and_value_errors_need_no_device():
    from parakeet_amd import audio
    x = np.zeros(40000, np.float32)
    with pytest.raises(NotImplementedError):
        audio.frame_power([x], frame_length=16385, hop_length=512)
    with pytest.raises(NotImplementedError):
        audio.frame_power([x], frame_length=400, hop_length=401)
    with pytest.raises(ValueError):
        audio.frame_power([x], frame_length=400, hop_length=0)
    with pytest.raises(ValueError):
        audio.trim(x, pad_mode="edge")
    with pytest.raises(ValueError):
        audio.trim(x[:1024])                                   # reflect needs more than 1024 samples
    with pytest.raises(ValueError):
        audio.trim_batch([x, x[:0]])
    kw = dict(vad_window_length=30, vad_moving_average_width=8, vad_max_silence_length=6, sampling_rate=16000)
    for bad, exc in ((dict(vad_moving_average_width=65), NotImplementedError), (dict(vad_max_silence_length=65), NotImplementedError),
                     (dict(vad_window_length=1100), NotImplementedError), (dict(vad_moving_average_width=0), ValueError),
                     (dict(vad_max_silence_length=-1), ValueError), (dict(vad_window_length=0), ValueError)):
        with pytest.raises(exc):
            audio.trim_long_silences(x, **dict(kw, **bad))
    assert audio.trim_num_frames(6000, 2048, 512) == 12 and audio.trim_num_frames(5, 6, 6, center=False) == 0
    assert (audio.TRIM_MAX_FRAME, audio.TRIM_MAX_AVG, audio.TRIM_MAX_SILENCE) == (16384, 64, 64)


def test_vad_none_is_the_preprocessor_of_before():
    from parakeet_amd import ge2e_audio
    rng = np.random.default_rng(3)
    wav = (0.01 * rng.standard_normal(16000)).astype(np.float32)
    want = ge2e_audio.normalize_volume(wav, -30, increase_only=True)
    for pre in (ge2e_audio.ge2e_preprocessor(), ge2e_audio.ge2e_preprocessor(vad=None)):
        assert pre.vad is None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                    # (the once-per-process "no webrtcvad" warning)
            got = pre.preprocess_wav(wav)
        assert got.dtype == want.dtype and np.array_equal(got, want) and not np.array_equal(got, wav)
    with pytest.raises(ValueError):
        ge2e_audio.ge2e_preprocessor(vad="webrtc")
    assert ge2e_audio.ge2e_preprocessor(vad="energy").vad == "energy"
    assert callable(ge2e_audio.ge2e_preprocessor(vad=lambda w: np.ones(len(w) // 480, bool)).vad)
