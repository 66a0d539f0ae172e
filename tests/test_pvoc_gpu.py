"""The phase vocoder, time stretching and pitch shifting on the engine (csrc/pvoc.hip) against the float64
restatement tests/pvoc_ref.py.  The engine is DEFINED operation by operation (csrc/pk_pvoc.h), so the comparisons of the
vocoder are ``==`` on float32 bits:

  * n_bin 17, 33, 65, 129 (below, at and one past a wave of 64 lanes, two waves plus one) x frames 1, 2, 3, 37, 300 x rates
    0.5, 2.0 (alpha exactly 0), 0.7, 1.0, 2^(1/12), 3.7 and a rate beyond the frame count; float32 noise with bins set exactly
    to zero and one whole frame zero (the u(0) = 1 rule, the zero columns past the end);
  * a ragged batch with a rate per utterance: the same bytes per utterance as alone, reversed, and at another position;
  * ``time_stretch_batch`` ``==`` the three stages called by hand, cropped and zero-padded;
  * a 440 Hz sine through ``time_stretch`` and ``pitch_shift``: lengths and the spectral peak within one analysis bin;
  * the C ABI's refusals, the example script in a child process."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pvoc_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3, 37, 300)
RATES = (0.5, 2.0, 0.7, 1.0, 1.0594630943592953, 3.7, None)      # None: a rate beyond the frame count, F + 2.5
_cache = {}


def _np(t):
    return t.as_subclass(torch.Tensor).detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _rows(n_bin, F):
    """(F, 2 * n_bin) float32 noise; bins 0, 5 and n_bin - 1 zero in every frame, a few single values zero, frame F // 2 zero"""
    key = ("rows", n_bin, F)
    if key not in _cache:
        rng = np.random.default_rng(1000 * n_bin + F)
        x = (3.0 * rng.standard_normal((F, 2 * n_bin))).astype(np.float32)
        for b in (0, 5, n_bin - 1):
            x[:, b] = 0
            x[:, n_bin + b] = 0
        x[::3, 7] = 0                                   # a zero real part alone is no zero bin
        x[1::4, 9] = 0
        x[1::4, n_bin + 9] = 0                          # bin 9 vanishes in every fourth frame
        if F >= 3:
            x[F // 2] = 0
        _cache[key] = x
    return _cache[key]


def _cases(n_bin):
    return [(_rows(n_bin, F), float(F) + 2.5 if r is None else r) for F in FRAMES for r in RATES]


def _want(n_bin):
    key = ("want", n_bin)
    if key not in _cache:
        _cache[key] = [R.phase_vocoder_rows(x, r) for x, r in _cases(n_bin)]
    return _cache[key]


@pytest.mark.parametrize("n_bin", [17, 33, 65, 129])
def test_engine_equals_the_restatement_as_bits(n_bin):
    from parakeet_amd import audio
    cases = _cases(n_bin)
    got = audio.phase_vocoder_batch([x for x, _ in cases], [r for _, r in cases])
    assert len(got) == len(cases) == 35
    for (x, r), g, w in zip(cases, got, _want(n_bin)):
        g = _np(g)
        assert g.dtype == np.float32 and g.shape == w.shape == (len(np.arange(0, x.shape[0], r)), 2 * n_bin), (n_bin, x.shape[0], r)
        bad = int((_bits(g) != _bits(w)).sum())
        assert bad == 0, (n_bin, x.shape[0], r, bad)
    assert _want(n_bin)[6].shape[0] == 1 and _want(n_bin)[-1].shape[0] == 1          # the rates beyond the frame count


def test_ragged_batches_give_the_same_bytes():
    from parakeet_amd import audio
    n_bin = 65
    cases = [(_rows(n_bin, F), r) for F, r in ((37, 0.7), (1, 0.5), (300, 1.0594630943592953), (3, 5.5), (2, 1.0), (37, 3.7),
                                               (300, 0.5))]
    alone = [_np(audio.phase_vocoder_batch([x], [r])[0]) for x, r in cases]
    for (x, r), a in zip(cases, alone):
        assert (_bits(a) == _bits(R.phase_vocoder_rows(x, r))).all()
    for order in (list(range(7)), list(range(7))[::-1], [3, 4, 5, 6, 0, 1, 2]):
        got = audio.phase_vocoder_batch([cases[i][0] for i in order], [cases[i][1] for i in order])
        for i, g in zip(order, got):
            assert _np(g).tobytes() == alone[i].tobytes(), (order, i)
    same = audio.phase_vocoder_batch([cases[0][0], cases[5][0]], 0.7)               # one number for the whole batch
    assert _np(same[0]).tobytes() == alone[0].tobytes()


def test_librosa_shaped_call():
    from parakeet_amd import audio
    x = _rows(33, 37)
    D = R.from_rows(x).astype(np.complex64)
    want = R.phase_vocoder_rows(x, 1.3)
    got = audio.phase_vocoder(D, 1.3, hop_length=8)
    assert isinstance(got, np.ndarray) and got.dtype == np.complex64 and got.shape == (33, want.shape[0])
    assert (_bits(got.real.T) == _bits(want[:, :33])).all() and (_bits(got.imag.T) == _bits(want[:, 33:])).all()
    t = audio.phase_vocoder(torch.from_numpy(D), 1.3, hop_length=512)               # hop_length has no effect
    assert isinstance(t, torch.Tensor) and t.dtype == torch.complex64 and t.shape == got.shape
    assert (_np(t) == got).all()


def test_time_stretch_is_its_three_stages():
    from parakeet_amd import audio
    n_fft, hop = 64, 16
    rng = np.random.default_rng(23)
    lens, rates = (1008, 1000, 1000, 517), (0.5, 0.7, 1.3, 2.0)
    wavs = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    got = audio.time_stretch_batch(wavs, rates, n_fft=n_fft, hop_length=hop)
    fwd, inv = audio._stretch_engines(n_fft, hop, n_fft, "hann", "dense")
    spec = fwd.run(wavs, 0)
    assert [s.shape[0] for s in spec] == [1 + n // hop for n in lens]
    pv = audio.phase_vocoder_batch(spec, rates)
    ys = inv.run(pv)
    sides = set()
    for n, r, g, s, p, y in zip(lens, rates, got, spec, pv, ys):
        T = R.num_frames(s.shape[0], r)
        assert p.shape[0] == T and y.shape[0] == hop * (T - 1)
        want_len = int(round(n / r))
        y, g = _np(y), _np(g)
        sides.add(want_len > len(y))
        want = y[:want_len] if len(y) >= want_len else np.concatenate([y, np.zeros(want_len - len(y), np.float32)])
        assert g.shape == (want_len,) and g.tobytes() == want.tobytes(), (n, r)
    assert sides == {True, False}                                                   # one is cropped, one is zero-padded
    one = audio.time_stretch(wavs[1], 0.7, n_fft=n_fft, hop_length=hop)
    assert _np(one).tobytes() == _np(got[1]).tobytes()
    fft = audio.time_stretch(wavs[1], 0.7, n_fft=n_fft, hop_length=hop, transform="fft")
    # another transform, the same effect.  Not a tight bar: where a bin nearly vanishes its phase is ill-conditioned and the
    # difference of the two transforms' roundings stays in the accumulated phase; 1e-2 of signals near 0.3 catches a wrong
    # pairing of the engines and nothing finer
    d = float(np.abs(_np(fft) - _np(one)).max())
    print(f"time_stretch, transform fft against dense: max difference {d:.3g}")
    assert fft.shape == one.shape and d <= 1e-2
    with pytest.raises(NotImplementedError):
        audio.time_stretch(wavs[0], 0.7, n_fft=60)                                  # the STFT's own limits, its own errors
    with pytest.raises(NotImplementedError):
        audio.time_stretch(wavs[0], 0.7, n_fft=64, hop_length=10)
    with pytest.raises(ValueError):
        audio.time_stretch(wavs[0][:20], 0.7, n_fft=64)                             # too short for reflect padding


SR, N, TONE = 8000, 4000, 440.0


def _sine():
    return np.sin(2 * np.pi * TONE * np.arange(N) / SR).astype(np.float32)


def test_stretched_sine_keeps_its_frequency():
    from parakeet_amd import audio
    rates = (0.8, 1.25, 2.0, 0.5)
    y = _sine()
    got = audio.time_stretch_batch([y] * 4, rates, n_fft=256, hop_length=64)
    for r, g in zip(rates, got):
        g = _np(g)
        assert g.shape == (int(round(N / r)),)
        hz, model = R.peak_hz(g, SR), R.peak_hz(R.time_stretch_model(y, r, 256, 64), SR)
        mid = g[len(g) // 4:len(g) - len(g) // 4]
        print(f"440 Hz sine stretched by rate {r}: {len(g)} samples, peak {hz:.3f} Hz (numpy model {model:.3f}), "
              f"RMS of the middle half {np.sqrt(np.mean(mid.astype(np.float64) ** 2)) / np.sqrt(0.5):.3f} of the input's")
        assert abs(hz - TONE) <= SR / 256 and abs(model - TONE) <= 1.0


@pytest.mark.parametrize("n_steps,want_hz", [(12, 880.0), (-12, 220.0)])
def test_pitch_shift_by_an_octave(n_steps, want_hz):
    from parakeet_amd import audio
    g = _np(audio.pitch_shift(_sine(), SR, n_steps, n_fft=256, hop_length=64))
    assert g.shape == (N,) and g.dtype == np.float32
    hz = R.peak_hz(g, SR)
    print(f"440 Hz sine shifted by {n_steps} steps: peak {hz:.3f} Hz")
    assert abs(hz - want_hz) <= SR / 256


def test_pitch_shift_by_nothing_returns_the_bits():
    from parakeet_amd import audio
    y = _sine()
    out = audio.pitch_shift_batch([y, y[:100]], SR, 0)
    assert _np(out[0]).tobytes() == y.tobytes() and _np(out[1]).tobytes() == y[:100].tobytes()
    assert _np(audio.pitch_shift(y, SR, 0.0, bins_per_octave=24)).tobytes() == y.tobytes()


def _refusal(status, code, word):
    from parakeet_amd import _capi
    assert status == code, (status, _capi.lib().pk_last_error())
    assert word in _capi.lib().pk_last_error().decode()


def test_c_abi_refusals():
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    lib = ctx.lib
    EINVAL, EUNSUP = -1, -3
    x, y = ctx.empty((4, 10)), ctx.empty((64, 10))
    i32 = lambda v: np.asarray(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    f64 = lambda v: np.asarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    run = lib.pk_pvoc_run
    _refusal(run(None, dptr(x), i32([4]), 1, 5, f64([1.0]), dptr(y)), EINVAL, "NULL")
    _refusal(run(ctx.handle, None, i32([4]), 1, 5, f64([1.0]), dptr(y)), EINVAL, "NULL")
    _refusal(run(ctx.handle, dptr(x), None, 1, 5, f64([1.0]), dptr(y)), EINVAL, "NULL")
    _refusal(run(ctx.handle, dptr(x), i32([4]), 1, 5, None, dptr(y)), EINVAL, "NULL")
    _refusal(run(ctx.handle, dptr(x), i32([4]), 1, 5, f64([1.0]), None), EINVAL, "NULL")
    _refusal(run(ctx.handle, dptr(x), i32([4]), 0, 5, f64([1.0]), dptr(y)), EINVAL, "batch")
    _refusal(run(ctx.handle, dptr(x), i32([4]), -3, 5, f64([1.0]), dptr(y)), EINVAL, "batch")
    _refusal(run(ctx.handle, dptr(x), i32([4]), 1, 0, f64([1.0]), dptr(y)), EINVAL, "n_bin")
    _refusal(run(ctx.handle, dptr(x), i32([2, 0]), 2, 5, f64([1.0, 1.0]), dptr(y)), EINVAL, "frames")
    _refusal(run(ctx.handle, dptr(x), i32([-4]), 1, 5, f64([1.0]), dptr(y)), EINVAL, "frames")
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        _refusal(run(ctx.handle, dptr(x), i32([2, 2]), 2, 5, f64([1.0, bad]), dptr(y)), EINVAL, "rate")
    _refusal(run(ctx.handle, dptr(x), i32([4]), 1, 5, f64([1e-9]), dptr(y)), EINVAL, "2^31")
    _refusal(run(ctx.handle, dptr(x), i32([4]), 1, 5, f64([5e-324]), dptr(y)), EINVAL, "2^31")      # frames / rate overflows
    many = np.ones(65536, np.int32)
    _refusal(run(ctx.handle, dptr(x), i32(many), 65536, 5, f64(np.ones(65536)), dptr(y)), EUNSUP, "65535")
    T = C.c_int64()
    _refusal(lib.pk_pvoc_num_frames(4, 1.0, None), EINVAL, "NULL")
    _refusal(lib.pk_pvoc_num_frames(0, 1.0, C.byref(T)), EINVAL, "frames")
    _refusal(lib.pk_pvoc_num_frames(4, float("nan"), C.byref(T)), EINVAL, "rate")
    _refusal(lib.pk_pvoc_num_frames(2 ** 31, 1.0, C.byref(T)), EINVAL, "2^31")
    assert lib.pk_pvoc_num_frames(2 ** 31 - 1, 1.0, C.byref(T)) == 0 and T.value == 2 ** 31 - 1
    assert lib.pk_pvoc_num_frames(5, 7.5, C.byref(T)) == 0 and T.value == 1


def test_example_script_in_a_child_process(tmp_path):
    """Three synthetic wavs of different lengths and sampling rates as one batch: slowed to rate 0.8 and shifted up an octave."""
    from parakeet_amd import audio
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    spec = {"a.wav": (8000, 4000, 440.0), "b.wav": (16000, 6001, 500.0), "c.wav": (22050, 5000, 1000.0)}
    for name, (sr, n, hz) in spec.items():
        audio.write_wav(str(src / name), (0.5 * np.sin(2 * np.pi * hz * np.arange(n) / sr)).astype(np.float32), sr, subtype="FLOAT")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "time_stretch.py"), "--in-dir", str(src), "--out-dir", str(dst),
                        "--rate", "0.8", "--n-steps", "12", "--n-fft", "256", "--hop-length", "64", "--subtype", "FLOAT"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 3
    for line, (name, (sr, n, hz)) in zip(lines, sorted(spec.items())):
        want_len = int(round(n / 0.8))
        assert line == f"{name}\t{sr}\t{n}\t{want_len}"
        wav, rate = audio.load_wav(str(dst / name))
        assert rate == sr and wav.shape == (want_len,)
        got = R.peak_hz(wav, sr)
        print(f"{name}: {n} -> {len(wav)} samples at {sr} Hz, peak {got:.2f} Hz (asked {2 * hz:.0f})")
        assert abs(got - 2 * hz) <= sr / 256
