"""Recursive filters, gated loudness and the gain kernel on the engine (csrc/iir.hip) against the float64
restatement tests/iir_ref.py.  The engine is DEFINED operation by operation (csrc/pk_iir.h), so the comparisons are ``==``:

  * filter outputs as bits, at every length around the chunk of 256 samples (1, 255, 256, 257, 511, 512, 513, 5 * 256 + 37)
    and 1, 2, 4 and 8 sections; the transition matrix the device computed ``==`` the restatement's; a burst followed by
    silence through a = [1, -0.5], whose state walks through the float64 subnormals to zero -- once as it is (the float32
    outputs reach zero long before) and once with a second section of gain 2^1000, which lifts the subnormal states into
    float32's range so that flushing them would show;
  * a ragged batch with an empty utterance: the same bytes per utterance as alone, reversed, and at another position;
  * pre-emphasis then de-emphasis: within the bound derived below;
  * every field of the loudness result ``==`` the restatement at 8 000 Hz (h = 800; lengths around 4 and 5 hop segments, and
    300 segments = 297 blocks, more than the 256 work items of the order over blocks) and at 22 050 Hz;
  * normalisation, the C ABI's refusals, the example script."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import iir_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (1, 255, 256, 257, 511, 512, 513, 5 * 256 + 37)
_cache = {}


def _np(t):
    return t.as_subclass(torch.Tensor).detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _filters():
    return {"deemph": R.lfilter_sos([1.0], [1.0, -0.97]), "k22050": R.k_weighting(22050),
            "butter8": signal.butter(8, 300, "hp", fs=22050, output="sos"),
            "butter16": signal.butter(16, 2000, "hp", fs=22050, output="sos")}


def _signals():
    if "sig" not in _cache:
        rng = np.random.default_rng(7)
        _cache["sig"] = [(0.1 * rng.standard_normal(L)).astype(np.float32) for L in LENGTHS]
    return _cache["sig"]


def _want(name):
    """the restatement's float32 outputs of every signal through filter `name`, computed once"""
    key = ("want", name)
    if key not in _cache:
        sos = _filters()[name]
        P = R.transition(sos)
        _cache[key] = [R.sosfilt(sos, x, P) for x in _signals()]
    return _cache[key]


@pytest.mark.parametrize("name,S", [("deemph", 1), ("k22050", 2), ("butter8", 4), ("butter16", 8)])
def test_filter_bits(name, S):
    from parakeet_amd import audio
    sos = _filters()[name]
    assert sos.shape == (S, 6)
    assert (audio._iir_engine(sos).transition() == R.transition(sos)).all()
    got = audio.sosfilt_batch(sos, _signals())
    for L, g, w in zip(LENGTHS, got, _want(name)):
        g = _np(g)
        assert g.shape == (L,) and g.dtype == np.float32
        assert (_bits(g) == _bits(w)).all(), (name, L, int((_bits(g) != _bits(w)).sum()))


def test_state_runs_through_the_subnormals():
    from parakeet_amd import audio
    x = np.zeros(64 + 1500, np.float32)
    x[:64] = (0.5 * np.random.default_rng(11).standard_normal(64)).astype(np.float32)
    one = R.lfilter_sos([1.0], [1.0, -0.5])
    w = R.sosfilt(one, x)
    g = _np(audio.lfilter([1.0], [1.0, -0.5], x))
    assert (_bits(g) == _bits(w)).all()
    lifted = np.concatenate([one, [[2.0 ** 1000, 0.0, 0.0, 1.0, 0.0, 0.0]]])
    w64 = R.sosfilt64(lifted, x)
    s = np.abs(w64[64 + 1030:64 + 1060]) / 2.0 ** 1000          # the first section's outputs there: float64 subnormals
    assert (s > 0).all() and (s < np.finfo(np.float64).tiny).all()
    with np.errstate(over="ignore"):                            # the burst itself times 2^1000 is beyond float32: inf on both sides
        w = w64.astype(np.float32)
    assert (np.abs(w[64 + 1030:64 + 1060]) > 0).all() and w[-1] == 0          # ... visible in float32, then gone
    g = _np(audio.sosfilt(lifted, x))
    assert (_bits(g) == _bits(w)).all()


def test_ragged_batches_give_the_same_bytes():
    from parakeet_amd import audio
    sos = _filters()["k22050"]
    sigs = _signals()
    alone = [_np(audio.sosfilt(sos, x)) for x in sigs]
    for a, w in zip(alone, _want("k22050")):
        assert (_bits(a) == _bits(w)).all()
    empty = np.zeros(0, np.float32)
    batch = sigs[:3] + [empty] + sigs[3:]
    got = [_np(g) for g in audio.sosfilt_batch(sos, batch)]
    assert got[3].shape == (0,)
    for g, a in zip(got[:3] + got[4:], alone):
        assert g.tobytes() == a.tobytes()
    got = [_np(g) for g in audio.sosfilt_batch(sos, batch[::-1])][::-1]
    for g, a in zip(got[:3] + got[4:], alone):
        assert g.tobytes() == a.tobytes()
    rolled = batch[5:] + batch[:5]                                   # every utterance at another position
    got = [_np(g) for g in audio.sosfilt_batch(sos, rolled)]
    got = got[-5:] + got[:-5]
    for g, a in zip(got[:3] + got[4:], alone):
        assert g.tobytes() == a.tobytes()
    assert _np(audio.sosfilt(sos, empty)).shape == (0,)


def test_preemphasis_then_deemphasis_returns_the_input():
    """p = fl32(pre(x)) carries a rounding error of at most half an ulp of max|p| per sample; de-emphasis is linear with the
    impulse response coef^n, whose 1-norm is 1 / (1 - coef), so that error reaches the output multiplied by at most that; the
    output's own rounding adds half an ulp of max|y|.  The float64 arithmetic inside adds terms of 2^-53 relative, covered by
    a relative 1e-12 of max|p| / (1 - coef)."""
    from parakeet_amd import audio
    coef = 0.97
    x = (0.3 * np.random.default_rng(13).standard_normal(5 * 256 + 37)).astype(np.float32)
    p = audio.preemphasis(x, coef)
    y = _np(audio.deemphasis(p, coef))
    p = _np(p)
    want_p = x.astype(np.float64)
    want_p[1:] = want_p[1:] - coef * x[:-1].astype(np.float64)
    assert (p == want_p.astype(np.float32)).all()
    pm, ym = np.abs(p).max(), max(np.abs(y).max(), np.abs(x).max())
    bound = (0.5 * float(np.spacing(np.float32(pm))) + 1e-12 * float(pm)) / (1.0 - coef) + 0.5 * float(np.spacing(np.float32(ym)))
    err = float(np.abs(y.astype(np.float64) - x.astype(np.float64)).max())
    print(f"pre-emphasis then de-emphasis: max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    ys = audio.deemphasis_batch(audio.preemphasis_batch([x, x[:300]], coef), coef)
    assert _np(ys[0]).tobytes() == y.tobytes() and _np(ys[1]).tobytes() == y[:300].tobytes()


def _loudness_inputs(sr, lengths):
    rng = np.random.default_rng(17)
    out = []
    for L in lengths:
        t = np.arange(L) / sr
        tone = np.sin(2 * np.pi * 440 * t)
        loud = (0.3 * tone + 0.05 * rng.standard_normal(L)).astype(np.float32)
        step = np.where(np.arange(L) < L // 2, 0.5, 0.005)
        out += [loud, (step * tone).astype(np.float32), (1e-4 * tone).astype(np.float32), np.zeros(L, np.float32)]
    return out


def _check_loudness(sr, xs):
    from parakeet_amd import metrics
    got = metrics.loudness_batch(xs, sr, return_details=True)
    lufs = metrics.loudness_batch(xs, sr)
    assert lufs.dtype == np.float64 and lufs.shape == (len(xs),)
    kept_some = dropped_some = silent = 0
    for i, (x, g) in enumerate(zip(xs, got)):
        w = R.loudness(x, sr)
        for field, ref in (("mean_power", "mean_power"), ("gated", "gated"), ("gated_abs", "gated_abs"), ("blocks", "blocks"),
                           ("relative_threshold_power", "rel")):
            assert g[field] == w[ref], (sr, i, len(x), field, g[field], w[ref])
        assert np.float32(g["peak"]) == w["peak"], (sr, i)
        assert g["lufs"] == w["lufs"] and lufs[i] == w["lufs"]            # numpy.log10 of the same float64 on both sides
        if w["rel"] > 0:
            assert g["relative_threshold_lufs"] == -0.691 + 10.0 * np.log10(w["rel"])
        kept_some += w["gated"] > 0
        dropped_some += 0 < w["gated"] < w["gated_abs"]
        silent += w["blocks"] > 0 and w["gated_abs"] == 0
    return kept_some, dropped_some, silent


def test_loudness_fields_at_8000():
    lengths = (3199, 3200, 3999, 4000, 4001, 8000 + 37, 300 * 800)
    xs = _loudness_inputs(8000, lengths)
    assert R.loudness(xs[-4], 8000)["blocks"] == 297                        # beyond the 256 work items of the order over blocks
    kept_some, dropped_some, silent = _check_loudness(8000, xs)
    assert kept_some >= 10 and dropped_some >= 2 and silent >= 10           # the inputs exercise both gates and the -inf results


def test_loudness_fields_at_22050_and_alone():
    from parakeet_amd import metrics
    L = int(1.2 * 22050)
    xs = _loudness_inputs(22050, (L,))
    kept_some, dropped_some, silent = _check_loudness(22050, xs)
    assert kept_some == 2 and dropped_some == 1 and silent == 2
    batch = metrics.loudness_batch(xs + [np.zeros(0, np.float32)], 22050, return_details=True)
    assert batch[-1]["lufs"] == -np.inf and batch[-1]["blocks"] == 0 and batch[-1]["peak"] == 0
    for x, b in zip(xs, batch):
        assert metrics.loudness_batch(x, 22050, return_details=True) == b     # alone: the same values
    assert metrics.loudness(xs[0], 22050) == batch[0]["lufs"]


def _normalisation_inputs(sr):
    rng = np.random.default_rng(19)
    n = 2 * sr
    t = np.arange(n) / sr
    return [(a * (np.sin(2 * np.pi * f * t) + 0.3 * rng.standard_normal(n))).astype(np.float32)
            for a, f in ((0.3, 220.0), (0.02, 440.0), (0.004, 880.0))]


def test_normalize_loudness():
    """The gain is rounded to float32 (a relative 2^-24, 5.2e-7 dB) and so is every scaled sample (each power term moves by a
    relative 2^-23 at most: 5.2e-7 dB on the mean); with the gate set unchanged -- asserted -- the re-measured loudness
    is the target within 1.1e-6 LU plus the float64 arithmetic.  The bar is 0.01 LU."""
    from parakeet_amd import audio, metrics
    sr = 16000
    xs = _normalisation_inputs(sr)
    short = xs[0][:4 * 1600 - 1].copy()                                 # one sample short of a block: -inf
    silent = np.zeros(sr, np.float32)
    before = metrics.loudness_batch(xs, sr, return_details=True)
    out, gains = audio.normalize_loudness_batch(xs + [short, silent], sr, -23.0, return_gains=True)
    assert gains.dtype == np.float32 and gains[3] == 1 and gains[4] == 1
    assert _np(out[3]).tobytes() == short.tobytes() and _np(out[4]).tobytes() == silent.tobytes()
    after = metrics.loudness_batch(out[:3], sr, return_details=True)
    for x, y, g, b, a in zip(xs, out, gains, before, after):
        assert (_np(y) == x * g).all()                                   # one float32 rounding per sample
        assert float(g) == float(np.float32(10.0 ** ((-23.0 - b["lufs"]) / 20.0)))
        assert (a["gated"], a["gated_abs"], a["blocks"]) == (b["gated"], b["gated_abs"], b["blocks"])
        print(f"normalised to -23: {b['lufs']:.4f} -> {a['lufs']:.6f} LUFS, gain {float(g):.6g}")
        assert abs(a["lufs"] - (-23.0)) <= 0.01
    capped, gains = audio.normalize_loudness_batch(xs, sr, -3.0, max_peak=0.5, return_gains=True)
    for x, y, g, b in zip(xs, capped, gains, before):
        assert float(np.abs(_np(y)).max()) <= 0.5
        assert float(g) <= 10.0 ** ((-3.0 - b["lufs"]) / 20.0) * (1 + 1e-7)
        assert float(np.abs(_np(y)).max()) > 0.4999                       # ... and the cap is what limited it
    y1, g1 = audio.normalize_loudness(xs[1], sr, -16.0, return_gains=True)
    assert abs(metrics.loudness(y1, sr) - (-16.0)) <= 0.01 and g1.dtype == np.float32


def _refusal(status, code, word):
    from parakeet_amd import _capi
    assert status == code, (status, _capi.lib().pk_last_error())
    assert word in _capi.lib().pk_last_error().decode()


def test_c_abi_refusals():
    from parakeet_amd import _capi, audio
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    lib = ctx.lib
    EINVAL, EUNSUP = -1, -3
    dp = C.POINTER(C.c_double)
    h = C.c_void_p()

    def create(rows, S):
        a = np.ascontiguousarray(rows, dtype=np.float64)
        return lib.pk_iir_create(ctx.handle, a.ctypes.data_as(dp), S, C.byref(h))

    good = [[1.0, 0.0, 0.0, 1.0, -0.5, 0.0]]
    _refusal(lib.pk_iir_create(ctx.handle, None, 1, C.byref(h)), EINVAL, "NULL")
    _refusal(create(good, 0), EINVAL, "sections")
    _refusal(create(good * 9, 9), EUNSUP, "sections")
    _refusal(create([[1.0, 0.0, 0.0, 2.0, -0.5, 0.0]], 1), EINVAL, "a0")
    _refusal(create([[1.0, np.inf, 0.0, 1.0, -0.5, 0.0]], 1), EINVAL, "finite")
    eng = audio._iir_engine(good)
    x, y = ctx.empty((16,)), ctx.empty((16,))
    i32 = lambda v: np.asarray(v, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    _refusal(lib.pk_iir_run(eng.h, None, i32([16]), 1, dptr(y)), EINVAL, "NULL")
    _refusal(lib.pk_iir_run(eng.h, dptr(x), i32([16]), 0, dptr(y)), EINVAL, "batch")
    many = np.zeros(65536, np.int32)
    _refusal(lib.pk_iir_run(eng.h, dptr(x), i32(many), 65536, dptr(y)), EUNSUP, "65535")
    _refusal(lib.pk_iir_run(eng.h, dptr(x), i32([4, -1]), 2, dptr(y)), EINVAL, "negative")
    _refusal(lib.pk_iir_run(eng.h, dptr(x), i32([2 ** 30 + 1]), 1, dptr(y)), EUNSUP, "samples")
    _refusal(lib.pk_iir_transition(eng.h, None), EINVAL, "NULL")
    m, r, c = ctx.empty((1,), torch.float64), ctx.empty((1,), torch.float64), ctx.empty((3,), torch.int32)
    for sr in (22051, 7990, 192010):
        _refusal(lib.pk_loudness_run(eng.h, dptr(x), i32([16]), 1, sr, dptr(m), dptr(r), dptr(y), dptr(c)), EUNSUP, "multiple of 10")
    _refusal(lib.pk_loudness_run(eng.h, dptr(x), i32([16]), 1, 16000, None, dptr(r), dptr(y), dptr(c)), EINVAL, "NULL")
    _refusal(lib.pk_loudness_run(eng.h, dptr(x), i32([-16]), 1, 16000, dptr(m), dptr(r), dptr(y), dptr(c)), EINVAL, "negative")
    g = np.ones(2, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    _refusal(lib.pk_gain_run(ctx.handle, dptr(x), i32([16]), 1, None, dptr(y)), EINVAL, "NULL")
    _refusal(lib.pk_gain_run(ctx.handle, dptr(x), i32([8, -8]), 2, g, dptr(y)), EINVAL, "negative")
    _refusal(lib.pk_gain_run(ctx.handle, dptr(x), i32([2 ** 30 + 1]), 1, g, dptr(y)), EUNSUP, "samples")
    with pytest.raises(ValueError):
        _capi.check(lib.pk_gain_run(ctx.handle, dptr(x), i32([16]), -1, g, dptr(y)))


def test_example_script_normalises_a_directory(tmp_path, capsys):
    """Written as PCM_16: the file's scale 32767 against the reader's 32768 costs 2.7e-4 dB and the quantisation noise
    (1 / 32768)^2 / 12 against a power near 5e-3 another 7e-8 dB, on top of the 1.1e-6 of ``test_normalize_loudness``."""
    from parakeet_amd import audio, metrics
    sr = 16000
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    for i, x in enumerate(_normalisation_inputs(sr)):
        audio.write_wav(str(src / f"utt{i}.wav"), x[:sr], sr, subtype="FLOAT")
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import normalize_loudness
    capsys.readouterr()
    normalize_loudness.main(["--in-dir", str(src), "--out-dir", str(dst), "--target", "-20", "--batch", "2"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 5 and lines[0].startswith("utt0.wav\t16000\t") and lines[3].startswith("loudness\t")
    assert lines[4].startswith("gain_db\t") and lines[4].endswith("over 3 files, target -20.000 LUFS")
    wavs = [audio.load_wav(str(dst / f"utt{i}.wav")) for i in range(3)]
    assert all(rate == sr for _, rate in wavs)
    got = metrics.loudness_batch([w for w, _ in wavs], sr)
    print("example script, files re-measured:", got)
    assert (np.abs(got - (-20.0)) <= 0.01).all()
