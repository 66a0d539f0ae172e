"""Silence trimming on the device (csrc/trim.hip) against the fp64 restatement of its definition (tests/trim_ref.py).

The frame power is compared on every frame under the relative bound ``eps_P`` derived from the kernel's stated accumulation
order; trim, split and the flags are integers and must be equal (tests/test_trim_cpu.py asserts that no frame of the signals
used here is within the power's error of a threshold, so equality is the whole test); everything after the voice detector
is a gather of the wav's own samples and is compared bit for bit with what the reference's source returned
(tests/golden/vad_post.npz).  A test asserts ratio <= 1 and prints it.

First hardware run (MI355X), largest ratio per test: see DESIGN.md 4.5f.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_bounds as fb  # noqa: E402
import trim_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vad_post.npz")
GE2E = (30, 8, 6, 16000)
MEL_MAX_REL = 1.2e-5       # the bound tests/test_speaker_encoder_gpu.py holds the GE2E power mel to


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------- 1. frame power
def _lengths(Lf, hop, T, mode):
    k = 5
    lens = [Lf // 2 + 1, Lf - 1, Lf, Lf + 1, k * hop - 1, k * hop, k * hop + 1]
    for frames in (T - 1, T, T + 1, 3 * T + 1):
        lens.append((frames - 1) * hop + Lf - 2 * (Lf // 2))   # the smallest N with that many frames
    if mode == "constant":
        lens += [1, 2]
    low = Lf // 2 + 1 if mode == "reflect" else 1
    return list(dict.fromkeys(n for n in lens if n >= low))


@pytest.mark.parametrize("mode", ["reflect", "constant"])
@pytest.mark.parametrize("Lf,hop", [(2048, 512), (1200, 300), (400, 160), (7, 3)])
def test_frame_power_every_frame(Lf, hop, mode):
    from parakeet_amd import audio
    T = audio.trim_tile_frames(Lf, hop)
    assert T >= 1
    lens = _lengths(Lf, hop, T, mode)
    got_frames = {tr.num_frames(n, Lf, hop) for n in lens}
    assert {T, T + 1, 3 * T + 1} <= got_frames and (T == 1 or T - 1 in got_frames)
    rng = np.random.default_rng(Lf + hop)
    content = [lambda n: tr.tone(n, phase=0.3), lambda n: rng.standard_normal(n).astype(np.float32),
               lambda n: np.zeros(n, np.float32), lambda n: np.full(n, 0.25, np.float32)]
    xs = [content[i % 4](n) for i, n in enumerate(lens)]
    xs += [c(max(lens)) for c in content] + [c(Lf + 1) for c in content]
    got = audio.frame_power(xs, Lf, hop, True, mode)
    root = audio.rms(xs, Lf, hop, True, mode)
    eps = tr.eps_P(Lf)
    worst = 0.0
    for x, g, r in zip(xs, got, root):
        want = tr.frame_power(x, Lf, hop, True, mode)
        g = _np(g)
        assert g.shape == want.shape == (tr.num_frames(x.size, Lf, hop),) and g.dtype == np.float32
        worst = max(worst, fb.ratio(g, want, eps * want))
        assert _same(_np(r), np.sqrt(g))                        # the square root is correctly rounded, like numpy's
    print(f"frame power {Lf}/{hop} {mode}: T {T}, {len(xs)} utterances of {min(lens)} ... {max(lens)} samples, ratio {worst:.4f} "
          f"(eps_P {eps:.3g})")
    assert worst <= 1.0
    # zeros give +0.0; a constant gives c^2 exactly where the frame holds no padding of zeros
    assert all(np.all(_np(g).view(np.uint32) == 0) for x, g in zip(xs, got) if not x.any())
    if mode == "reflect":
        assert all(np.all(_np(g) == np.float32(0.0625)) for x, g in zip(xs, got) if np.all(x == 0.25))


def test_frame_power_at_the_envelope():
    """frames longer than half the small LDS budget (one frame per tile), longer than all of it (the large budget) and the
    longest the engine takes; hop 1"""
    from parakeet_amd import audio
    rng = np.random.default_rng(9)
    worst = 0.0
    for Lf, hop, n in ((8192, 512, 20000), (8193, 1, 8500), (16384, 4096, 40000), (16384, 16384, 40000), (1, 1, 300)):
        T = audio.trim_tile_frames(Lf, hop)
        xs = [rng.standard_normal(n).astype(np.float32), tr.tone(n - 7)]
        for center, mode in ((True, "reflect"), (False, None)):
            got = audio.frame_power(xs, Lf, hop, center, mode or "reflect")
            for x, g in zip(xs, got):
                want = tr.frame_power(x, Lf, hop, center, mode or "reflect")
                assert want.size > 0
                worst = max(worst, fb.ratio(_np(g), want, tr.eps_P(Lf) * want))
        print(f"frame power {Lf}/{hop}: T {T}, ratio so far {worst:.4f}")
    assert worst <= 1.0
    short = audio.frame_power([np.ones(5, np.float32), np.ones(3, np.float32)], 6, 6, center=False)   # no frame at all
    assert [p.numel() for p in short] == [0, 0]


# ------------------------------------------------------------------------------------------------- 2. trim and split
@pytest.mark.parametrize("top_db", [20, 60])
def test_trim_and_split_equal_the_restatement(top_db):
    from parakeet_amd import audio
    cases = tr.trim_cases()
    names = sorted(cases)
    out, index = audio.trim_batch([cases[n] for n in names], top_db=top_db)
    flags = audio.nonsilent_frames_batch([cases[n] for n in names], top_db=top_db)
    assert index.shape == (len(names), 2) and index.dtype == np.int64
    for i, n in enumerate(names):
        x = cases[n]
        want = tr.trim_index(x, top_db)
        assert np.array_equal(index[i], want), (n, index[i], want)
        assert np.array_equal(_np(flags[i]), tr.nonsilent(tr.frame_power(x), top_db)), n
        assert isinstance(out[i], np.ndarray) and np.shares_memory(out[i], x) and _same(out[i], x[want[0]:want[1]])
        y, idx = audio.trim(x, top_db=top_db)
        assert np.array_equal(idx, want) and np.shares_memory(y, x)
        s = audio.split(x, top_db=top_db)
        assert s.dtype == np.int64 and np.array_equal(s, tr.split_index(x, top_db)), (n, s)
    assert tuple(index[names.index("zeros")]) == (0, 6000)
    assert index[names.index("to_last_sample")][1] == cases["to_last_sample"].size
    assert audio.split(cases["bursts"], top_db=top_db).shape == (3, 2)
    print(f"trim / split at top_db {top_db}: {len(names)} signals, every index equal")


def test_trim_of_a_device_tensor_is_a_view_of_it():
    from parakeet_amd import audio
    from parakeet_amd.runtime import Context
    x = tr.trim_cases()["lead_trail"]
    t = Context.get().to_device(x)
    y, idx = audio.trim(t)
    assert np.array_equal(idx, tr.trim_index(x)) and y.data_ptr() == t.data_ptr() + 4 * int(idx[0]) and y.numel() == idx[1] - idx[0]


# ------------------------------------------------------------------------------------- 3. any batch, any position
def test_any_batch_any_position_changes_no_bit():
    from parakeet_amd import audio
    cases = tr.trim_cases()
    x = cases["bursts"]
    v, _ = tr.burst_signal(seed=1)
    others = [cases["lead_trail"], cases["impulse"], tr.tone(12345), cases["zeros"]]
    ms, W, S, sr = GE2E

    def everything(batch, at, sig, vsig):
        P = _np(audio.frame_power(batch(sig), 2048, 512)[at])
        Pc = _np(audio.frame_power(batch(sig), 1200, 300, True, "constant")[at])
        Pn = _np(audio.frame_power(batch(sig), 480, 480, center=False)[at])
        fl = _np(audio.nonsilent_frames_batch(batch(sig), top_db=20)[at])
        idx = audio.trim_batch(batch(sig), top_db=20)[1][at]
        vad = _np(audio.trim_long_silences_batch(batch(vsig), ms, W, S, sr)[at])
        Q, vf = audio.energy_voice_flags_batch(batch(vsig), ms, sr)[at]
        nrm = _np(audio.peak_normalize_batch(batch(sig))[at])
        return [P, Pc, Pn, fl, idx, vad, _np(Q), _np(vf), nrm]

    alone = everything(lambda s: [s], 0, x, v)
    assert alone[0].size > 2 * audio.trim_tile_frames(2048, 512) and alone[5].size > 0
    for at in (0, 2, 4):
        def batch(s, at=at):
            b = list(others)
            b.insert(at, s)
            return b
        got = everything(batch, at, x, v)
        for k, (a, g) in enumerate(zip(alone, got)):
            assert _same(a, g), (at, k)
    # center=False windows are summed in the order of the centred frames that cover the same samples
    Lf = 480
    cen = _np(audio.frame_power([x], Lf, Lf, True, "constant")[0])
    unc = _np(audio.frame_power([x[Lf // 2:]], Lf, Lf, center=False)[0])
    assert unc.size >= 10 and _same(unc, cen[1:1 + unc.size])
    print("alone and at positions 0, 2, 4 of five: power (three geometries), flags, bounds, VAD output, detector, peak: same bits")


# ---------------------------------------------------------------------------------------------- 4. after the detector
def test_after_the_detector_is_the_references_bit_for_bit():
    from parakeet_amd import audio
    cases = tr.vad_golden(GOLDEN)
    groups = {}
    for c in cases:
        groups.setdefault((c["ms"], c["W"], c["S"], c["sr"]), []).append(c)
    n = 0
    for (ms, W, S, sr), cs in sorted(groups.items()):       # one ragged call per parameter set
        got = audio.trim_long_silences_batch([c["wav"] for c in cs], ms, W, S, sr, voice_flags=[c["flags"] for c in cs])
        for c, g in zip(cs, got):
            assert _same(_np(g), c["out"]), c["name"]
            n += 1
    assert n == len(cases)
    print(f"{n} golden cases in {len(groups)} ragged calls: bit for bit")


def test_scan_chunk_edges_and_an_utterance_shorter_than_a_window():
    from parakeet_amd import _capi, audio
    ch = _capi.PK_TRIM_SCAN_CHUNK
    rng = np.random.default_rng(11)
    w, W, S = 4, 8, 6
    wavs, flags = [], []
    for n_w in (ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 3, 1, 0):
        wavs.append(rng.uniform(-1, 1, n_w * w + 3).astype(np.float32))
        f = np.repeat(rng.uniform(size=n_w // 6 + 1) < 0.5, 6)[:n_w]
        if n_w >= ch:                                       # runs and gaps across the chunk boundary
            f[ch - 9:ch - 2] = True
            f[ch - 2:ch + 5] = False
            f[ch + 5:ch + 9] = True
        flags.append(f)
    got = audio.trim_long_silences_batch(wavs, 4, W, S, 1000, voice_flags=flags)
    for x, f, g in zip(wavs, flags, got):
        assert _same(_np(g), tr.trim_long_silences(x, f, w, W, S)), f.size
    assert got[-1].numel() == 0 and got[-1].dtype == got[0].dtype
    # the widest average and dilation the engine takes
    g = audio.trim_long_silences_batch(wavs[:5], 4, 64, 64, 1000, voice_flags=flags[:5])
    assert all(_same(_np(a), tr.trim_long_silences(x, f, w, 64, 64)) for a, x, f in zip(g, wavs, flags))
    only_short = audio.trim_long_silences_batch([wavs[-1]], 4, W, S, 1000)
    assert only_short[0].numel() == 0
    with pytest.raises(ValueError):
        audio.trim_long_silences(wavs[0], 4, W, S, 1000, voice_flags=flags[0][:-1])


# ---------------------------------------------------------------------------------------------- 5. the energy detector
def test_energy_detector_flags_and_the_five_window_result():
    from parakeet_amd import audio
    ms, W, S, sr = GE2E
    w = tr.window_size(ms, sr)
    gaps = (6, 9, 14, 25)
    sigs = [tr.burst_signal(gaps=gaps, seed=s) for s in (0, 1)]
    det = audio.energy_voice_flags_batch([x for x, _ in sigs], ms, sr)
    out = audio.trim_long_silences_batch([x for x, _ in sigs], ms, W, S, sr)
    worst = 0.0
    for (x, built), (Q, f), o in zip(sigs, det, out):
        Qr, fr, thr = tr.energy_flags(x, w)
        dec = tr.decided_windows(Qr, thr, tr.eps_P(w))
        worst = max(worst, fb.ratio(_np(Q), Qr, tr.eps_P(w) * Qr))
        assert dec.all() and np.array_equal(_np(f)[dec], fr[dec]) and np.array_equal(fr, built)
        assert _same(_np(o), tr.trim_long_silences(x, fr, w, W, S))
        # end to end: every interior silence is five windows long in the result
        Qo, fo = audio.energy_voice_flags_batch([o], ms, sr)[0]
        silent = tr.runs(~_np(fo))
        assert [b - a for a, b in silent if a > 0 and b < fo.numel()] == [5] * len(gaps)
    print(f"energy detector: window power ratio {worst:.4f}, flags equal on every (decided) window, silences of {gaps} -> 5")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ 6. GE2E
def test_ge2e_preprocessor_with_the_energy_detector():
    from parakeet_amd import ge2e_audio
    import ge2e_ref
    x, built = tr.pause_signal()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain, none, energy = (ge2e_audio.ge2e_preprocessor(), ge2e_audio.ge2e_preprocessor(vad=None),
                               ge2e_audio.ge2e_preprocessor(vad="energy"))
        given = ge2e_audio.ge2e_preprocessor(vad=lambda wav: built)
        w_plain, w_none, w_energy, w_given = (p.preprocess_wav(x) for p in (plain, none, energy, given))
    assert _same(w_plain, w_none)                              # vad=None: the bits of the call without the argument
    p_plain, p_none = (_np(p.extract_mel_partials(wv)) for p, wv in ((plain, w_plain), (none, w_none)))
    assert _same(p_plain, p_none)
    norm = ge2e_audio.normalize_volume(x, -30, increase_only=True).astype(np.float32)
    ms, W, S, sr = GE2E
    want = tr.trim_long_silences(norm, tr.energy_flags(norm, tr.window_size(ms, sr))[1], tr.window_size(ms, sr), W, S)
    assert w_energy.dtype == np.float32 and _same(w_energy, want) and _same(w_given, want)
    got = _np(energy.extract_mel_partials(w_energy))
    _, sl = ge2e_audio.compute_partial_slices(len(want), 160, 160, 0.75, 0.5)
    pad = np.pad(want, (0, max(0, 160 * sl[-1].stop - len(want))))
    ref = ge2e_ref.mel_partials(pad, [s.start for s in sl]).numpy()
    rel = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"vad='energy': {got.shape[0]} partials (untrimmed {p_plain.shape[0]}), power mel relative error {rel:.3e}, "
          f"ratio {rel / MEL_MAX_REL:.4f}")
    assert got.shape == ref.shape and rel / MEL_MAX_REL <= 1.0
    assert got.shape[0] < p_plain.shape[0]


# -------------------------------------------------------------------------------------------------- 7. peak normalise
def test_peak_normalize_bit_for_bit():
    from parakeet_amd import _capi, audio
    rng = np.random.default_rng(2)
    tile = 16384
    xs = [rng.standard_normal(n).astype(np.float32) * np.float32(s)
          for n, s in ((1, 1.0), (3, 0.1), (tile - 1, 3.0), (tile, 1e-3), (tile + 1, 7.0), (3 * tile + 5, 0.5), (1001, 1e-30))]
    xs.insert(3, np.zeros(777, np.float32))                      # all zero: unchanged
    xs.append(np.full(100, 1e-39, np.float32))                   # max below the smallest normal: unchanged
    big = rng.standard_normal(5000).astype(np.float32)
    big[4999] = -9.0                                             # the peak is negative and last
    xs.append(big)
    got = audio.peak_normalize_batch(xs)
    for x, g in zip(xs, got):
        assert _same(_np(g), tr.peak_normalize(x)), x.size
    assert _same(_np(got[3]), xs[3]) and _same(_np(got[-2]), xs[-2]) and _np(got[-1])[4999] == -1.0
    assert _same(_np(audio.peak_normalize(xs[5])), tr.peak_normalize(xs[5]))
    assert _capi.PK_TRIM_SCAN_CHUNK == 256
