"""The resampler's definition and its host side, without a device: the fp64 reference (tests/resample_ref.py) against
scipy's polyphase filter given the same taps, ``resample_filter`` against the formula, lengths, the envelope, ``load_wav``."""
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as rr  # noqa: E402

PAIRS = [(48000, 22050), (44100, 16000), (16000, 22050), (22050, 44100), (22050, 16000)]


def _lm(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
@pytest.mark.parametrize("sr_in,sr_out,N", [p + (130,) for p in PAIRS] + [(48000, 16000, 1), (16000, 48000, 1)])
def test_reference_is_scipy_polyphase_with_these_taps(sr_in, sr_out, N, res_type):
    """h[k] = g(k / L) / L handed to scipy.signal.resample_poly (which multiplies given taps by ``up``) is the direct sum."""
    import scipy.signal
    L, M = _lm(sr_in, sr_out)
    zeros, rolloff, beta = rr.FILTERS[res_type]
    half = int(math.ceil(zeros * max(L, M)))
    h = rr.g_of_q(np.arange(-half, half + 1), L, M, zeros, rolloff, beta) / L
    x = np.random.default_rng(N + L).normal(size=N)
    want = scipy.signal.resample_poly(x, L, M, window=h)
    got = rr.resample_ref(x, L, M, res_type)
    assert got.shape == want.shape == (rr.out_len(N, L, M),)
    err = float(np.abs(got - want).max())
    print(f"{sr_in}->{sr_out} {res_type}: max |direct sum - resample_poly| = {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
@pytest.mark.parametrize("L,M", [(147, 320), (441, 320), (2, 1), (1, 3), (160, 441), (1, 1)])
def test_filter_rows_are_g_at_the_documented_taps(L, M, res_type):
    from parakeet_amd.audio import resample_filter, resample_taps
    zeros, rolloff, beta = rr.FILTERS[res_type]
    tab = resample_filter(L, M, res_type)
    T = resample_taps(L, M, zeros)
    H = T // 2
    assert tab.shape == (L, T) and tab.dtype == np.float64 and H == math.ceil(zeros * max(L, M) / L)
    # row p, tap k: g(H - 1 - k + p / L), i.e. q = (H - 1 - k) L + p
    q = (H - 1 - np.arange(T))[None, :] * L + np.arange(L)[:, None]
    want = rr.g_of_q(q, L, M, zeros, rolloff, beta)
    assert np.abs(tab - want).max() <= 1e-15
    outside = np.abs(q) >= zeros * max(L, M)               # |s tau| >= zeros
    assert outside.any() and np.all(tab[outside] == 0.0)
    # the taps left out on either side (k = -1 and k = T) are outside the support for every phase
    for k in (-1, T):
        assert np.all(np.abs((H - 1 - k) * L + np.arange(L)) >= zeros * max(L, M))
    # explicit parameters override the named set
    t2 = resample_filter(L, M, res_type, zeros=8, rolloff=0.8, beta=5.0)
    assert t2.shape == (L, resample_taps(L, M, 8))
    q2 = (t2.shape[1] // 2 - 1 - np.arange(t2.shape[1]))[None, :] * L + np.arange(L)[:, None]
    assert np.abs(t2 - rr.g_of_q(q2, L, M, 8, 0.8, 5.0)).max() <= 1e-15


def test_filter_table_reproduces_the_direct_sum():
    """y[n] = sum_k table[(n M) mod L][k] x[floor(n M / L) - (H - 1) + k]: the layout the engine is handed."""
    from parakeet_amd.audio import resample_filter
    for L, M in ((147, 320), (441, 320), (3, 1), (1, 12)):
        x = np.random.default_rng(L).normal(size=97)
        tab = resample_filter(L, M, "kaiser_fast")
        H = tab.shape[1] // 2
        xp = np.concatenate([np.zeros(H), x, np.zeros(H + M)])
        n = np.arange(rr.out_len(97, L, M))
        y = np.array([tab[(i * M) % L] @ xp[i * M // L + 1:i * M // L + 1 + 2 * H] for i in n])
        assert np.abs(y - rr.resample_ref(x, L, M, "kaiser_fast")).max() <= 1e-13


def test_output_length_is_the_ceiling():
    from parakeet_amd.audio import Resample, resample_ratio
    for sr_in, sr_out in PAIRS + [(48000, 16000), (16000, 48000), (96000, 8000)]:
        L, M = _lm(sr_in, sr_out)
        assert resample_ratio(sr_in, sr_out) == (L, M)
        rs = Resample.__new__(Resample)                    # the length rule needs no device
        rs.up, rs.down = L, M
        seen = set()
        for N in range(1, 4 * M + 2):
            assert rs.output_length(N) == math.ceil(N * L / M) == rr.out_len(N, L, M)
            seen.add(N * L % M)
        assert {0, 1 % M, M - 1} <= seen
    big = 13_700_000
    rs.up, rs.down = 160, 441
    assert rs.output_length(big) == (big * 160 + 440) // 441


def test_envelope_refusals_name_their_limit():
    from parakeet_amd.audio import Resample, resample_filter
    with pytest.raises(NotImplementedError, match="4096"):
        Resample(22050, 22051)
    with pytest.raises(NotImplementedError, match="4096"):
        Resample(22051, 22050)
    with pytest.raises(NotImplementedError, match="8192"):
        Resample(48000, 1000, zeros=128)                   # 2 * 128 * 48 = 12288 taps
    with pytest.raises(NotImplementedError, match=str(4 << 20)):
        Resample(4000, 4001, zeros=600)                    # 4001 phases of 1200 taps
    with pytest.raises(ValueError):
        Resample(16000, 8000, res_type="sinc_best")
    with pytest.raises(ValueError):
        Resample(0, 8000)
    with pytest.raises(ValueError):
        resample_filter(0, 3)


def test_standard_rates_are_inside_the_envelope():
    from parakeet_amd.audio import (RESAMPLE_MAX_TABLE, RESAMPLE_MAX_TAPS, _check_resample_envelope, resample_ratio,
                                    resample_taps)
    rates = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000)
    worst = 0
    for a in rates:
        for b in rates:
            if a != b:
                L, M = resample_ratio(a, b)
                T = resample_taps(L, M, 64)
                _check_resample_envelope(L, M, T)
                assert L <= 1280 and T <= RESAMPLE_MAX_TAPS and L * T <= RESAMPLE_MAX_TABLE
                worst = max(worst, L * T)
    print("largest table of the standard rates:", worst, "coefficients")


def _riff(fmt_tag, ch, rate, bits, body, extensible=False):
    block = ch * bits // 8
    if extensible:
        sub = struct.pack("<H", fmt_tag) + bytes.fromhex("000000001000800000aa00389b71")
        fmt = struct.pack("<HHIIHH", 0xFFFE, ch, rate, rate * block, block, bits) + struct.pack("<HHI", 22, bits, 0) + sub
    else:
        fmt = struct.pack("<HHIIHH", fmt_tag, ch, rate, rate * block, block, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"LIST" + struct.pack("<I", 3) + b"abc\0"   # an odd chunk, padded
    chunks += b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def _int_bytes(v, bits):
    if bits == 8:
        return (v + 128).astype(np.uint8).tobytes()
    if bits == 16:
        return v.astype("<i2").tobytes()
    if bits == 32:
        return v.astype("<i4").tobytes()
    b = v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]
    return np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("extensible", [False, True])
@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_load_wav_integer_pcm(tmp_path, bits, extensible):
    from parakeet_amd.audio import load_wav
    rng = np.random.default_rng(bits)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    v = rng.integers(lo, hi + 1, size=(301, 2), dtype=np.int64)
    v[0], v[1] = (lo, hi), (hi, lo)
    p = tmp_path / "x.wav"
    p.write_bytes(_riff(1, 2, 44100, bits, _int_bytes(v.reshape(-1), bits), extensible))
    wav, sr = load_wav(p)
    want = (v.astype(np.float64).mean(axis=1) / (1 << (bits - 1)))
    assert sr == 44100 and wav.dtype == np.float32 and wav.shape == (301,)
    assert np.abs(wav - want).max() <= 2.0 ** -24           # one float32 rounding of values in [-1, 1]
    st, _ = load_wav(p, mono=False)
    assert st.shape == (2, 301)
    assert np.abs(st - v.T.astype(np.float64) / (1 << (bits - 1))).max() <= 2.0 ** -25
    one, _ = load_wav(_riff(1, 1, 8000, bits, _int_bytes(v[:, 0], bits), extensible))      # bytes, mono
    assert np.array_equal(one, st[0])
    same, sr2 = load_wav(p, sr=44100)                       # the file's own rate: no resampling, no device
    assert sr2 == 44100 and np.array_equal(same, wav)


def test_load_wav_float32_and_what_write_wav_writes(tmp_path):
    from parakeet_amd.audio import load_wav, write_wav
    x = np.random.default_rng(0).uniform(-1, 1, size=(257, 2)).astype(np.float32)
    write_wav(tmp_path / "f.wav", x, 32000, subtype="FLOAT")
    st, sr = load_wav(tmp_path / "f.wav", mono=False)
    assert sr == 32000 and np.array_equal(st, x.T)
    mono, _ = load_wav(tmp_path / "f.wav")
    assert np.array_equal(mono, x.mean(axis=1))
    (tmp_path / "e.wav").write_bytes(_riff(3, 2, 32000, 32, x.astype("<f4").tobytes(), extensible=True))
    assert np.array_equal(load_wav(tmp_path / "e.wav", mono=False)[0], x.T)
    write_wav(tmp_path / "p.wav", x[:, 0], 22050)
    back, sr = load_wav(tmp_path / "p.wav")
    assert sr == 22050 and np.array_equal(back, np.rint(x[:, 0] * 32767.0).astype(np.float32) / 32768.0)
    with pytest.raises(NotImplementedError, match="format tag"):
        load_wav(_riff(6, 1, 8000, 8, b"\0" * 16))          # A-law
    with pytest.raises(ValueError, match="RIFF"):
        load_wav(b"RIFX" + b"\0" * 40)


def test_read_wav_same_rate_16_bit_values_are_unchanged(tmp_path):
    """A 16-bit file at the processor's rate gives the values of the code path it replaces, recomputed here from the bytes:
    int16 -> float32, mean over the channels, / 32768, then the peak normalisation."""
    import wave
    from parakeet_amd.audio import AudioProcessor
    v = np.random.default_rng(5).integers(-32768, 32768, size=(400, 2)).astype("<i2")
    p = tmp_path / "s.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(22050)
        w.writeframes(v.tobytes())
    with wave.open(str(p), "rb") as w:
        raw = w.readframes(w.getnframes())
    want = np.frombuffer(raw, dtype="<i2").astype(np.float32).reshape(-1, 2).mean(axis=1) / 32768.0
    ap = AudioProcessor.__new__(AudioProcessor)              # read_wav needs the rate and the flag only
    ap.sample_rate, ap.normalize = 22050, False
    got = ap.read_wav(p)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    ap.normalize = True
    assert np.array_equal(ap.read_wav(p), want / np.max(np.abs(want)) * 0.999)


def test_numpy_resample_of_equal_rates_needs_no_device():
    from parakeet_amd.audio import resample
    x = np.random.default_rng(1).normal(size=100).astype(np.float32)
    y = resample(x, 22050, 22050)
    assert y is not x and y.dtype == np.float32 and np.array_equal(y.view(np.uint32), x.view(np.uint32))


def _tone(f, res_type="kaiser_best"):
    """(amplitude of the f Hz sine in the output by a least-squares fit, rms of the output / rms of the input) for a unit sine,
    300 output samples away from the ends.  (The fit, not the rms, measures the pass band: the rms of a sine over a window that
    is not a whole number of periods is off by about 1 / (4 pi periods) on its own.)"""
    L, M = _lm(48000, 22050)
    N = 4800
    x = np.sin(2 * np.pi * f * np.arange(N) / 48000.0 + 0.3)
    y = rr.resample_ref(x, L, M, res_type)
    t = np.arange(y.size)[300:-300] / 22050.0
    y = y[300:-300]
    basis = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], 1)
    amp = float(np.hypot(*np.linalg.lstsq(basis, y, rcond=None)[0]))
    return amp, float(np.sqrt(np.mean(y * y)) / np.sqrt(np.mean(x * x)))


def test_tones_through_the_reference_48k_to_22k05():
    """What the definition does to sines (conditions the fp64 reference meets, 300 samples away from the ends): the pass band
    is flat, everything above the new Nyquist frequency is gone."""
    for f in (1000.0, 8000.0):
        gain = _tone(f)[0]
        print(f"{f:.0f} Hz: gain {gain:.6f}")
        assert abs(gain - 1.0) <= 1e-3
    for f in (12000.0, 14000.0, 20000.0):
        gain = _tone(f)[1]
        print(f"{f:.0f} Hz: {gain:.3g} of the input rms")
        assert gain <= 1e-6
