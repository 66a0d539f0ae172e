"""STOI / ESTOI on the engine (csrc/stoi.hip) against the float64 restatement tests/stoi_ref.py, stage by
stage and as a whole, through ``parakeet_amd.metrics``.  Everything is at 10 kHz unless a test says otherwise.

  * mask: ``==`` the restatement's.  Condition on the inputs, asserted here on the CPU side: no frame lies within 0.01 dB of the
    threshold (a float32 sum of 256 squares moves e by under 1e-4 dB).
  * bands: ``stoi_ref.band_bound`` -- the forward bound tests/rfft_ref.py derives for n = 512, carried through the range sum
    and the square root.
  * segments: engine against numpy on the same float32 bands, ``stoi_ref.stoi_seg_bound`` / ``estoi_seg_bound`` (operation
    count, 1 ulp for the double sqrt); the inputs are conditioned (kappa <= 100, centred column norms >= 0.05), asserted.
  * whole pipeline, both variants, one ragged batch: the tolerance is ten times the largest difference between the fp32
    evaluation of the plan (``stoi_ref.stoi_f32``) and the float64 restatement on these same inputs (the README's
    regression-bar convention; it covers the engine's different fp32 summation order).  That difference is measured on the CPU
    inside the test and asserted to be what this docstring records: 7.28e-7 (STOI 4.72e-7, ESTOI 7.28e-7), so the tolerance is
    7.28e-6.  The engine's first measured error on the MI355X against the restatement: STOI 4.43e-7, ESTOI 5.72e-7
    (bands 0.034 of their bound, segments 5e-6 of theirs).
  * every utterance alone, in the batch and in the reversed batch: the same bytes.
  * 16 000 and 22 050 Hz: against the restatement run on the engine's own resampled signals (the resampler is not what is
    tested), same tolerance.
The lengths: 4096, 4097, 4225 (0, 1, 2 segments, nothing removed), the constructed silences of the issue, 30 000, and kept-frame
counts at every tile size of the kernels and one either side: 4 frames per workgroup of the energy kernel and of the FFT at
n = 512, 4 segments per wave and 16 per workgroup of the segment kernel (K - 30 segments), 256 frames per scan step of the mask
kernel, 256 segments per step of the reduction."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))
import stoi_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN_DB = 0.01
PLAN_DIFF = 7.28e-7               # the module docstring's figure; the test asserts the measured one is within 20 % of it
TILE_K = (3, 4, 5, 33, 34, 35, 45, 46, 47, 255, 256, 257, 285, 286, 287)
_cache = {}


def _np(t):
    return t.as_subclass(torch.Tensor).detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _zeroed(L, seed, spans):
    x = sr.harmonic(L, seed)
    for a, b in spans:
        x[a:b] = 0.0
    return x


def _cases():
    """name -> dict(x, y, all_kept): the inputs of every test, their float64 results computed once."""
    if "cases" in _cache:
        return _cache["cases"]
    raw = [("L4096", sr.harmonic(4096, 0), True), ("L4097", sr.harmonic(4097, 0), True), ("L4225", sr.harmonic(4225, 0), True),
           ("gap5324", _zeroed(5324, 1, [(2000, 3024)]), False), ("lead6000", _zeroed(6000, 2, [(0, 1000)]), False),
           ("gaps9000", _zeroed(9000, 3, [(0, 300), (4000, 5500)]), False), ("L30000", sr.harmonic(30000, 4), True)]
    for K in TILE_K:
        L = 257 + 128 * (K - 1) + (37 * K) % 128
        assert sr.num_frames(L) == K
        raw.append((f"K{K}", sr.harmonic(L, 10 + K), True))
    cases = {}
    for i, (name, x, all_kept) in enumerate(raw):
        y = sr.add_noise(x, (20, 10, 5, 0)[i % 4], i)
        keep, _ = sr.silent_mask(x)
        assert sr.threshold_margin(x) >= MARGIN_DB, (name, sr.threshold_margin(x))     # the condition on the inputs
        assert bool(keep.all()) == all_kept, name
        cases[name] = dict(x=x, y=y, keep=keep)
    _cache["cases"] = cases
    return cases


def _want(extended):
    key = ("want", extended)
    if key not in _cache:
        _cache[key] = {n: sr.stoi(c["x"], c["y"], extended) for n, c in _cases().items()}
    return _cache[key]


def _tolerance():
    """10 x the largest |fp32 plan - float64 restatement| over the cases and both variants, measured here"""
    if "tol" not in _cache:
        worst = {}
        for ext in (False, True):
            w = 0.0
            for n, c in _cases().items():
                a, b = sr.stoi_f32(c["x"], c["y"], ext), _want(ext)[n]
                assert (a["segments"], a["kept"], a["frames"]) == (b["segments"], b["kept"], b["frames"]), n
                if b["segments"]:
                    w = max(w, abs(a["d"] - b["d"]))
            worst[ext] = w
        diff = max(worst.values())
        print(f"STOI-PLAN fp32 plan against float64: STOI {worst[False]:.3e}, ESTOI {worst[True]:.3e}")
        assert 0.8 * PLAN_DIFF <= diff <= 1.2 * PLAN_DIFF, diff
        _cache["tol"] = 10.0 * diff
    return _cache["tol"]


def test_mask_equals_the_restatement():
    from parakeet_amd import metrics
    cases = _cases()
    got = metrics.stoi_silent_frames([c["x"] for c in cases.values()])
    for (name, c), (keep, e) in zip(cases.items(), got):
        assert keep.dtype == bool and keep.shape == c["keep"].shape, name
        assert np.array_equal(keep, c["keep"]), name
        _, e64 = sr.silent_mask(c["x"])
        assert np.max(np.abs(e - e64)) <= 1e-3 if len(e) else True, name            # information: dB, float32 sums and rounding
    # the frames wholly inside the constructed silences are removed (one reaching into the signal by a few samples of the
    # window's edge may be as well: tests/test_stoi_cpu.py has the case where the rest is kept exactly)
    g = cases["gaps9000"]["keep"]
    starts = np.arange(len(g)) * sr.HOP
    inside = ((starts + sr.FRAME <= 300) | ((starts >= 4000) & (starts + sr.FRAME <= 5500)))
    assert not g[inside].any() and inside.sum() >= 10 and g.sum() >= len(g) - inside.sum() - 4


def test_bands_within_the_rfft_bound():
    from parakeet_amd import metrics
    cases = _cases()
    names = ["L4097", "gap5324", "K3", "K4", "K5", "K33", "K257"]
    got = metrics.stoi_bands([cases[n]["x"] for n in names] + [np.zeros(300, np.float32), np.zeros(100, np.float32)])
    worst = 0.0
    for n, g in zip(names, got):
        x = cases[n]["x"]
        want = sr.bands(x)
        g = _np(g).astype(np.float64)
        assert g.shape == want.shape == (sr.num_frames(len(x)), sr.J), n
        bound = sr.band_bound(x, want)
        assert np.all(g[bound == 0] == 0)                    # frames of exact zeros: zero bands, no tolerance
        worst = max(worst, float((np.abs(g - want)[bound > 0] / bound[bound > 0]).max()))
    print(f"SWEEP-RATIO stoi bands against float64, rfft_bound through the range sum and the root: {worst:.4f}")
    assert worst <= 1.0
    assert worst > 1e-4                                      # the comparison is not vacuous
    assert _np(got[-2]).shape == (1, sr.J) and not _np(got[-2]).any() and _np(got[-1]).shape == (0, sr.J)


def _band_inputs():
    """Conditioned float32 band matrices: entries in [0.1, 1) (kappa about 2.5), the degraded ones a noisy, partly clipped copy."""
    out = []
    for i, F in enumerate((0, 1, 29, 30, 31, 32, 33, 34, 35, 44, 45, 46, 47, 284, 285, 286, 287, 600)):
        r = np.random.default_rng([F, i])
        x = r.uniform(0.1, 1.0, (F, sr.J)).astype(np.float32)
        y = (x * r.uniform(0.6, 1.4, (F, sr.J)) + r.uniform(0.0, 0.3, (F, sr.J))).astype(np.float32)
        y[r.uniform(size=(F, sr.J)) < 0.05] *= np.float32(12.0)        # entries the clipping of STOI acts on
        out.append((x, y))
    return out


@pytest.mark.parametrize("extended", [False, True])
def test_segments_against_numpy_on_the_same_bands(extended):
    from parakeet_amd import metrics
    pairs = _band_inputs()
    got = metrics.stoi_from_bands([x for x, _ in pairs], [y for _, y in pairs], extended)
    worst = 0.0
    for (x, y), (d, S) in zip(pairs, got):
        want, Sw, info = sr.segments(x, y, extended, details=True)
        assert S == Sw == max(x.shape[0] - 29, 0)
        if S == 0:
            assert np.isnan(d) and np.isnan(want)
            continue
        assert info["kappa"] <= 100.0, info                          # the condition on the inputs
        if extended:
            assert info["cmin"] >= 0.05, info
        bound = sr.estoi_seg_bound(100.0, 0.05, S) if extended else sr.stoi_seg_bound(100.0, S)
        assert bound < 1e-8
        worst = max(worst, abs(d - want) / bound)
    print(f"SWEEP-RATIO stoi segments (extended={extended}) against numpy float64: {worst:.6f}")
    assert worst <= 1.0
    # the same pair alone gives the same bytes
    x, y = pairs[-1]
    assert np.float64(metrics.stoi_from_bands(x, y, extended)[0]).tobytes() == np.float64(got[-1][0]).tobytes()


@pytest.mark.parametrize("extended", [False, True])
def test_whole_pipeline_ragged_batch(extended):
    from parakeet_amd import metrics
    cases, want, tol = _cases(), _want(extended), _tolerance()
    assert tol <= 1e-5
    got = metrics.stoi_batch([c["x"] for c in cases.values()], [c["y"] for c in cases.values()], sr.FS, extended,
                             return_details=True)
    worst = 0.0
    for (name, c), g in zip(cases.items(), got):
        w = want[name]
        assert (g["segments"], g["kept_frames"], g["frames"]) == (w["segments"], w["kept"], w["frames"]), name
        if w["segments"] == 0:
            assert np.isnan(g["d"]) and np.isnan(w["d"]), name
            continue
        worst = max(worst, abs(g["d"] - w["d"]))
    print(f"STOI-ENGINE extended={extended}: largest |engine - float64| {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol
    assert want["L4096"]["segments"] == 0 and want["L4097"]["segments"] == 1 and want["L4225"]["segments"] == 2
    assert want["gap5324"]["kept"] < want["gap5324"]["frames"]
    # the scores order with the noise: a cleaner copy of the same signal scores higher
    x = cases["L30000"]["x"]
    d = metrics.stoi_batch([x] * 3, [sr.add_noise(x, s, 99) for s in (20, 5, -10)], sr.FS, extended)
    assert d[0] > d[1] > d[2]


@pytest.mark.parametrize("extended", [False, True])
def test_identical_signals_and_silence(extended):
    from parakeet_amd import metrics
    cases, tol = _cases(), _tolerance()
    names = ["L4097", "gaps9000", "L30000", "K257"]
    got = metrics.stoi_batch([cases[n]["x"] for n in names], [cases[n]["x"] for n in names], sr.FS, extended)
    for n, d in zip(names, got):
        assert abs(d - 1.0) <= tol, (n, d)
    # an all-zero clean signal: every frame is kept, every band is zero, the result is finite and the restatement's
    z = np.zeros(6000, np.float32)
    g = metrics.stoi_batch([z, z], [z, cases["lead6000"]["y"]], sr.FS, extended, return_details=True)
    for gi, y in zip(g, (z, cases["lead6000"]["y"])):
        w = sr.stoi(z, y, extended)
        assert np.isfinite(gi["d"]) and gi["d"] == w["d"] == 0.0
        assert (gi["segments"], gi["kept_frames"], gi["frames"]) == (w["segments"], w["kept"], w["frames"]) == (15, 45, 45)


@pytest.mark.parametrize("extended", [False, True])
def test_same_bytes_alone_in_the_batch_and_reversed(extended):
    from parakeet_amd import metrics
    cases = _cases()
    xs, ys = [c["x"] for c in cases.values()], [c["y"] for c in cases.values()]
    key = lambda r: (np.float64(r["d"]).tobytes(), r["segments"], r["kept_frames"], r["frames"])  # noqa: E731
    batch = [key(r) for r in metrics.stoi_batch(xs, ys, sr.FS, extended, return_details=True)]
    rev = [key(r) for r in metrics.stoi_batch(xs[::-1], ys[::-1], sr.FS, extended, return_details=True)][::-1]
    assert batch == rev
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert key(metrics.stoi_batch(x, y, sr.FS, extended, return_details=True)) == batch[i], list(cases)[i]
    assert metrics.stoi(xs[-1], ys[-1], sr.FS, extended) == metrics.stoi_batch(xs, ys, sr.FS, extended)[-1]


@pytest.mark.parametrize("rate", [16000, 22050])
def test_other_rates_go_through_the_engines_resampler(rate):
    from parakeet_amd import audio, metrics
    tol = _tolerance()
    L = int(0.9 * rate)
    r = np.random.default_rng(rate)
    t = np.arange(L) / rate
    x = (0.3 * (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t)) * sum(np.sin(2 * np.pi * 150.0 * k * t + k) / k for k in range(1, 9))
         + 1e-3 * r.normal(size=L)).astype(np.float32)
    y = (x + 0.05 * r.normal(size=L)).astype(np.float32)
    rs = audio.Resample(rate, sr.FS)
    x10, y10 = (_np(v) for v in rs.run_batch([x, y]))
    assert sr.threshold_margin(x10) >= MARGIN_DB
    for ext in (False, True):
        g = metrics.stoi_batch(x, y, rate, ext, return_details=True)
        w = sr.stoi(x10, y10, ext)
        assert (g["segments"], g["kept_frames"], g["frames"]) == (w["segments"], w["kept"], w["frames"]) and w["segments"] > 0
        assert abs(g["d"] - w["d"]) <= tol, (ext, g["d"], w["d"])
        assert 0.0 < g["d"] < 1.0


def test_score_vocoder_example_prints_stoi(tmp_path, capsys):
    """``examples/score_vocoder.py --stoi`` on a directory pair: a pair of unequal length is truncated to the shorter signal,
    the columns are ``stoi_batch``'s on that pair, the corpus means follow."""
    from parakeet_amd import audio, metrics
    import score_vocoder as ex
    rate = 16000
    c = _cases()["L30000"]
    rs = audio.Resample(sr.FS, rate)
    x, y = (_np(v) for v in rs.run_batch([c["x"], c["y"]]))
    (tmp_path / "ref").mkdir()
    (tmp_path / "gen").mkdir()
    audio.write_wav(str(tmp_path / "ref" / "a.wav"), x, rate, subtype="FLOAT")
    audio.write_wav(str(tmp_path / "gen" / "a.wav"), y[:-700], rate, subtype="FLOAT")
    audio.write_wav(str(tmp_path / "ref" / "b.wav"), x[:20000], rate, subtype="FLOAT")
    audio.write_wav(str(tmp_path / "gen" / "b.wav"), x[:20000], rate, subtype="FLOAT")
    capsys.readouterr()
    ex.main(["--gen-dir", str(tmp_path / "gen"), "--ref-dir", str(tmp_path / "ref"), "--stoi"])
    lines = capsys.readouterr().out.strip().split("\n")
    a, b = lines[0].split("\t"), lines[1].split("\t")
    assert a[0] == "a" and int(a[1]) == len(y) - 700 and "trimmed" in lines[0] and b[0] == "b"
    n = len(y) - 700
    want = [metrics.stoi(x[:n], y[:n], rate, ext) for ext in (False, True)]
    assert [float(a[4]), float(a[5])] == [float(f"{w:.6f}") for w in want] and 0.0 < want[1] < want[0] < 1.0
    assert abs(float(b[4]) - 1.0) < 1e-5 and abs(float(b[5]) - 1.0) < 1e-5
    assert lines[-2].startswith("stoi\t") and lines[-1].startswith("estoi\t") and lines[-1].endswith("over 2 utterances")
    assert abs(float(lines[-2].split("\t")[1]) - (want[0] + float(b[4])) / 2) < 2e-6
