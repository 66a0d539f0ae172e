"""The radix FFT on the engine (csrc/rfft.hip): ``audio.rfft`` / ``audio.irfft`` against numpy.fft in fp64 under the bound
derived in tests/rfft_ref.py, the STFT / ISTFT / Griffin-Lim on ``transform="fft"`` under that bound carried through the
existing ones, dense against FFT, batch invariance bit for bit, and the surface.  ``SWEEP-RATIO`` lines give error / bound.
"""
import ctypes as C
import functools
import math
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import fp32_bounds as fb
import istft_ref as ir
import rfft_ref as rr
import sweep_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = rr.fft_cfgs()


def _np(t):
    return t.detach().cpu().numpy()


def _rows(D):
    return np.ascontiguousarray(ir.reim(D), dtype=np.float32)


def _cplx(rows):
    nb = rows.shape[1] // 2
    return rows[:, :nb].astype(np.float64) + 1j * rows[:, nb:].astype(np.float64)


@functools.lru_cache(maxsize=None)
def _fwd(c, transform="fft", power=False, mel=False, log_base=0):
    from parakeet_amd.audio import _Engine, mel_filterbank
    basis = mel_filterbank(c.sr, c.n_fft, c.n_mels, sc.MEL_FMIN, sc.MEL_FMAX) if mel else None
    return _Engine(c.n_fft, c.hop, c.win, "hann", c.center, power, basis, log_base, transform=transform)


@functools.lru_cache(maxsize=None)
def _inv(c, transform="fft"):
    from parakeet_amd.audio import _InvEngine
    return _InvEngine(c.n_fft, c.hop, c.win, "hann", c.center, transform=transform)


def _run(eng, wavs, what):
    return [_np(o) for o in eng.run(wavs, what)]


def _tap(eng, what, frames, nb):
    from parakeet_amd import _capi
    out = np.empty((frames, 2 * nb), np.float32)
    _capi.check(eng.ctx.lib.pk_gl_debug_read(eng.h, what, _capi.fptr(out), out.size))
    return out


# ------------------------------------------------------------------------------------------------ 1. / 2. rows
def _row_ratio(got, want, b):
    nb = want.shape[1]
    return max(fb.ratio(got[:, :nb], want.real, b), fb.ratio(got[:, nb:], want.imag, b))


@pytest.mark.parametrize("n", rr.SIZES)
def test_rfft_rows(n):
    from parakeet_amd import audio
    T = audio.rfft_tile_rows(n)
    worst = 0.0
    for rows in rr.tile_row_counts(T):
        for name, x in rr.row_inputs(n, rows).items():
            got = _np(audio.rfft(x))
            assert got.shape == (rows, n + 2) and got.dtype == np.float32
            want = np.fft.rfft(x.astype(np.float64), axis=1)
            worst = max(worst, _row_ratio(got, want, rr.rfft_bound(np.abs(x.astype(np.float64)), n)))
            if name == "silence":
                assert not got.any()
            if name == "impulse":
                assert np.abs(np.abs(_cplx(got)) - 1.0).max() <= rr.rfft_c(n) * fb.U
            if name == "nyquist":
                assert got[0, n // 2] == n
    print(f"SWEEP-RATIO rfft n{n} {worst:.4g}")
    assert worst <= 1.0
    # a row's spectrum is the same bits wherever it stands; the complex view holds the same numbers
    x = rr.row_inputs(n, T + 1)["gaussian"]
    full = _np(audio.rfft(x))
    assert np.array_equal(_np(audio.rfft(x[-1:])), full[-1:]) and np.array_equal(_np(audio.rfft(x[:1])), full[:1])
    cx = _np(audio.rfft(x, as_complex=True))
    assert cx.dtype == np.complex64 and cx.shape == (T + 1, n // 2 + 1)
    assert np.array_equal(cx.real, full[:, :n // 2 + 1]) and np.array_equal(cx.imag, full[:, n // 2 + 1:])


@pytest.mark.parametrize("n", rr.SIZES)
def test_irfft_rows(n):
    from parakeet_amd import audio
    T = audio.rfft_tile_rows(n)
    worst = worst_rt = 0.0
    for rows in rr.tile_row_counts(T):
        for name, x in rr.row_inputs(n, rows).items():
            X = np.fft.rfft(x.astype(np.float64), axis=1).astype(np.complex64)
            got = _np(audio.irfft(rr.reim(X)))
            assert got.shape == (rows, n) and got.dtype == np.float32
            want = np.fft.irfft(X.astype(np.complex128), n=n, axis=1)
            worst = max(worst, fb.ratio(got, want, rr.irfft_bound(rr.absspec(X), n)))
            if name == "silence":
                assert not got.any()
            # round trip on the device: the inverse sees the forward's spectrum, whose bins are off by at most e; through
            # the linear inverse that is (e + e + 2 (n/2 - 1) e) / n = e per sample, on top of the inverse's own bound
            spec = audio.rfft(x)
            back = _np(audio.irfft(spec))
            e = rr.rfft_bound(np.abs(x.astype(np.float64)), n)
            lim = e + rr.irfft_bound(rr.absspec(_cplx(_np(spec))), n)
            worst_rt = max(worst_rt, fb.ratio(back, x.astype(np.float64), lim))
    print(f"SWEEP-RATIO irfft n{n} {worst:.4g}")
    print(f"SWEEP-RATIO rfft_round_trip n{n} {worst_rt:.4g}")
    assert worst <= 1.0 and worst_rt <= 1.0
    # NaN in im(DC) and im(Nyquist) is never read; complex input is the same rows
    r = np.random.default_rng(n)
    X = (r.normal(0, 1, (T + 1, n // 2 + 1)) + 1j * r.normal(0, 1, (T + 1, n // 2 + 1))).astype(np.complex64)
    rows = rr.reim(X)
    base = _np(audio.irfft(rows))
    bad = rows.copy()
    bad[:, n // 2 + 1] = np.nan
    bad[:, -1] = np.nan
    got = _np(audio.irfft(bad, n=n))
    assert np.all(np.isfinite(got)) and np.array_equal(got, base)
    assert np.array_equal(_np(audio.irfft(X)), base) and np.array_equal(_np(audio.irfft(torch.from_numpy(X))), base)
    assert fb.ratio(base, np.fft.irfft(X.astype(np.complex128), n=n, axis=1), rr.irfft_bound(rr.absspec(X), n)) <= 1.0
    assert np.array_equal(_np(audio.irfft(rows[-1:])), base[-1:])


# ------------------------------------------------------------------------------------------------ 3. STFT
@functools.lru_cache(maxsize=None)
def _stft_case(c):
    wavs = sc.mel_batch(c)
    return wavs, _run(_fwd(c), wavs, 0)


@pytest.mark.parametrize("c", CFGS, ids=sc.mel_id)
def test_stft_on_the_fft_path(c):
    from parakeet_amd.audio import mel_filterbank
    basis = mel_filterbank(c.sr, c.n_fft, c.n_mels, sc.MEL_FMIN, sc.MEL_FMAX).astype(np.float64)
    wavs, reim = _stft_case(c)
    nb = 1 + c.n_fft // 2
    got = {"reim": reim, "mag": _run(_fwd(c), wavs, 1), "pow": _run(_fwd(c, power=True), wavs, 1),
           "mel": _run(_fwd(c, mel=True), wavs, 2), "log10": _run(_fwd(c, mel=True, log_base=10), wavs, 2),
           "energy": _run(_fwd(c), wavs, 3)}
    frames = [sc.num_frames(c, len(w)) for w in wavs]
    assert c.total_frames is None or sum(frames) == c.total_frames
    worst = {k: 0.0 for k in got}
    unusable = 0
    floor = sc.MEL_FLOOR
    for u, w in enumerate(wavs):
        for k in got:
            assert got[k][u].shape[0] == frames[u], (k, u)
        if frames[u] == 0:
            continue
        ref = rr.stft_fft(w, c)
        re, im = ref["spec"].real, ref["spec"].imag
        b = np.broadcast_to(ref["bound"], re.shape)
        worst["reim"] = max(worst["reim"], fb.ratio(got["reim"][u][:, :nb], re, b), fb.ratio(got["reim"][u][:, nb:], im, b))
        mag, b_mag = np.hypot(re, im), fb.magnitude_bound(re, im, b, b)
        worst["mag"] = max(worst["mag"], fb.ratio(got["mag"][u], mag, b_mag))
        pw, b_pw = re * re + im * im, fb.power_bound(re, im, b, b)
        worst["pow"] = max(worst["pow"], fb.ratio(got["pow"][u], pw, b_pw))
        mel, b_mel = mag @ basis.T, fb.mel_bound(np.abs(basis), mag, b_mag, nb)
        worst["mel"] = max(worst["mel"], fb.ratio(got["mel"][u], mel, b_mel))
        b10, usable = fb.log_bound(mel, b_mel, floor, math.log(10.0))
        worst["log10"] = max(worst["log10"], fb.ratio(got["log10"][u], np.log10(np.maximum(mel, floor)), b10, usable))
        unusable += int((~usable).sum())
        # energy = sqrt(max(sum_k |X_k|^2, floor)): the power bound per bin, n_bin additions ((n_bin + 2) u with spare), and
        # |sqrt(a') - sqrt(a)| <= |a' - a| / sqrt(a) with sqrtf's own rounding (2u: not assumed correctly rounded)
        E = pw.sum(1, keepdims=True)
        b_E = b_pw.sum(1, keepdims=True) + (nb + 2) * fb.U * (E + b_pw.sum(1, keepdims=True))
        loud = E - b_E > floor
        if loud.any():
            lim = b_E / np.sqrt(np.where(loud, E, 1.0)) + 2.0 * fb.U * np.sqrt(E)
            worst["energy"] = max(worst["energy"], fb.ratio(got["energy"][u], np.sqrt(E), lim, loud))
    for k, v in worst.items():
        print(f"SWEEP-RATIO stft_fft {sc.mel_id(c)} {k} {v:.4g}")
    assert max(worst.values()) <= 1.0
    assert unusable < 0.01 * sum(frames) * c.n_mels
    for k in ("reim", "mag", "pow", "mel"):                              # silence (utterance 1) is exactly zero
        assert not got[k][1].any()
    z = got["energy"][1]
    assert np.array_equal(z, np.full_like(z, z[0, 0])) and abs(float(z[0, 0]) - math.sqrt(floor)) <= 2.0 * fb.U * math.sqrt(floor)


# ------------------------------------------------------------------------------------------------ 4. ISTFT
@functools.lru_cache(maxsize=None)
def _istft_case(c):
    specs = ir.sweep_spectra(c)
    rows = [_rows(D) for D in specs]
    return specs, rows, [_np(o) for o in _inv(c).run(rows)]


@pytest.mark.parametrize("c", CFGS, ids=sc.mel_id)
def test_istft_on_the_fft_path(c):
    from parakeet_amd import _capi
    specs, rows, got = _istft_case(c)
    eng = _inv(c)
    worst = worst_raw = 0.0
    for D, y in zip(specs, got):
        assert y.shape == (ir.num_samples(c, D.shape[0]),)
        ref = rr.istft_fft(D, c)
        divided = ref["env"] > ir.FLT_MIN
        worst = max(worst, fb.ratio(y, ref["wav"], ref["bound"], divided))
        worst_raw = max(worst_raw, fb.ratio(y, ref["raw"], ref["bound"], ~divided))
    print(f"SWEEP-RATIO istft_fft {sc.mel_id(c)} divided {worst:.4g}")
    print(f"SWEEP-RATIO istft_fft {sc.mel_id(c)} undivided {worst_raw:.4g}")
    assert worst <= 1.0 and worst_raw <= 1.0
    assert not got[1].any()                                              # silence stays silence
    # NaN in the imaginary parts of DC and Nyquist does not reach the samples
    nb = 1 + c.n_fft // 2
    bad = rows[-1].copy()
    bad[:, nb] = np.nan
    bad[:, -1] = np.nan
    assert np.array_equal(_np(eng.run([bad])[0]), got[-1])
    # PK_HOST_IO, bit for bit
    frames = np.array([r.shape[0] for r in rows], dtype=np.int32)
    x = np.ascontiguousarray(np.concatenate(rows), dtype=np.float32)
    out = np.full(sum(eng.samples(f) for f in frames), np.nan, np.float32)
    _capi.check(eng.ctx.lib.pk_istft_run(eng.h, _capi.fptr(x), frames.ctypes.data_as(C.POINTER(C.c_int32)), len(rows),
                                         _capi.fptr(out), _capi.PK_HOST_IO))
    assert np.array_equal(out, np.concatenate(got))


# ------------------------------------------------------------------------------------------------ 5. dense against FFT
@pytest.mark.parametrize("c", CFGS, ids=sc.mel_id)
def test_dense_and_fft_agree(c):
    """Both paths write the same layout: their results differ by at most the sum of their bounds, without a reference in
    between (the fp64 values only size the bounds)."""
    wavs, fft = _stft_case(c)
    dense = _run(_fwd(c, "dense"), wavs, 0)
    nb = 1 + c.n_fft // 2
    worst = 0.0
    for w, a, d in zip(wavs, fft, dense):
        assert a.shape == d.shape
        if a.shape[0] == 0:
            continue
        lim = np.tile(rr.stft_fft(w, c)["bound"], (1, 2 * nb)) + sc.mel_reference(c, w, np.zeros((1, nb)))["b_reim"]
        worst = max(worst, fb.ratio(a, d.astype(np.float64), lim))
    print(f"SWEEP-RATIO dense_vs_fft {sc.mel_id(c)} stft {worst:.4g}")
    assert worst <= 1.0
    specs, rows, got = _istft_case(c)
    B = ir.synthesis_basis(c)
    worst = 0.0
    for D, r, y in zip(specs, rows, got):
        d = _np(_inv(c, "dense").run([r])[0])
        lim = rr.istft_fft(D, c)["bound"] + ir.istft(D, c, with_bound=True, basis=B)["bound"]
        worst = max(worst, fb.ratio(y, d.astype(np.float64), lim))
    print(f"SWEEP-RATIO dense_vs_fft {sc.mel_id(c)} istft {worst:.4g}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 6. batch invariance
@pytest.mark.parametrize("c", CFGS, ids=sc.mel_id)
def test_batch_invariance_bit_for_bit(c):
    wavs, reim = _stft_case(c)
    fwd, inv = _fwd(c), _inv(c)
    for u, w in enumerate(wavs):
        if reim[u].shape[0] == 0:                                         # shorter than a frame: nothing to transform alone
            continue
        others = [x for v, x in enumerate(wavs) if v != u][:3]
        assert np.array_equal(_run(fwd, [w], 0)[0], reim[u]), ("stft alone", u)
        assert np.array_equal(_run(fwd, [w] + others, 0)[0], reim[u]), ("stft first", u)
        assert np.array_equal(_run(fwd, others + [w], 0)[-1], reim[u]), ("stft last", u)
    _, rows, got = _istft_case(c)
    for u, r in enumerate(rows):
        others = [x for v, x in enumerate(rows) if v != u][:3]
        assert np.array_equal(_np(inv.run([r])[0]), got[u]), ("istft alone", u)
        assert np.array_equal(_np(inv.run([r] + others)[0]), got[u]), ("istft first", u)
        assert np.array_equal(_np(inv.run(others + [r])[-1]), got[u]), ("istft last", u)


@pytest.mark.parametrize("c", ir.GL_CFGS, ids=sc.mel_id)
def test_griffin_lim_batch_invariance(c):
    S32 = _gl_case(c)[0]
    fwd, inv = _fwd(c), _inv(c)
    other, third = np.ascontiguousarray(S32[:7] * 0.5), np.ascontiguousarray(S32[2:] * 2.0)

    def run(mags, seeds):
        return [_np(o) for o in inv.griffin_lim(fwd, mags, 4, 0.99, seeds)]

    a = run([S32], [7])[0]
    assert np.all(np.isfinite(a))
    assert np.array_equal(a, run([S32, other, third], [7, 3, 4])[0])
    assert np.array_equal(a, run([other, third, S32], [3, 4, 7])[-1])


# ------------------------------------------------------------------------------------------------ 7. Griffin-Lim
@functools.lru_cache(maxsize=None)
def _gl_case(c):
    S, a0 = ir.gl_problem(c)
    S32 = S.astype(np.float32)
    ang = _rows(a0)
    nb = S.shape[1]
    return S32, ang, S32.astype(np.float64), ang[:, :nb].astype(np.float64) + 1j * ang[:, nb:].astype(np.float64)


@pytest.mark.parametrize("c", ir.GL_CFGS, ids=sc.mel_id)
def test_griffin_lim_one_step(c):
    S32, ang, S64, a64 = _gl_case(c)
    F, nb = S32.shape
    eng, fwd = _inv(c), _fwd(c)
    ref = ir.griffin_lim(S64, c, 1, 0.99, a64)
    wav = _np(eng.griffin_lim(fwd, [S32], 1, 0.99, None, [ang])[0])
    rebuilt, iterate = _tap(eng, 0, F, nb), _tap(eng, 1, F, nb)
    assert np.array_equal(wav, _np(eng.run([iterate])[0]))               # the waveform is the ISTFT of the tapped iterate

    # the rebuilt spectrum: x0 = istft(S * angles0) carries the inverse's bound, the forward transform adds its own
    x0 = rr.istft_fft(S64 * a64, c)
    b_reb = np.broadcast_to(rr.stft_fft(x0["wav"], c, x_err=x0["bound"])["bound"], ref["rebuilt"].shape)
    r1 = float((np.abs(_cplx(rebuilt) - ref["rebuilt"]) / b_reb).max())
    print(f"SWEEP-RATIO gl_fft_one_step {sc.mel_id(c)} rebuilt {r1:.4g}")
    assert r1 <= 1.0

    # the update from shared angles where |rebuilt| is tiny (ill-conditioned phase): the restatement alone decides which
    mag = np.abs(ref["rebuilt"])
    excl = mag < 1e-3 * mag.max()
    share = excl.mean()
    print(f"SWEEP-INFO gl_fft_one_step {sc.mel_id(c)} excluded_share {share:.4f}")
    assert share <= 0.05
    want_spec = S64 * ref["angles"]
    X = _cplx(iterate)
    X[excl] = want_spec[excl]
    X = X.astype(np.complex64)
    e = np.where(excl, 2.0 * fb.U * S64, S64 * b_reb / np.where(excl, 1.0, mag))
    lim = rr.istft_fft(want_spec, c, err=e)
    r2 = fb.ratio(_np(eng.run([_rows(X)])[0]), lim["wav"], lim["bound"])
    print(f"SWEEP-RATIO gl_fft_one_step {sc.mel_id(c)} wav {r2:.4g}")
    assert r2 <= 1.0
    assert wav.shape == lim["wav"].shape and np.all(np.isfinite(wav))


@pytest.mark.parametrize("c", ir.GL_CFGS, ids=sc.mel_id)
def test_griffin_lim_whole_run(c):
    S32, ang, S64, a64 = _gl_case(c)
    F, nb = S32.shape
    eng, fwd = _inv(c), _fwd(c)
    ref = ir.griffin_lim(S64, c, 32, 0.99, a64, keep=(4, 32))
    sc4, sc32 = (ir.spectral_convergence(ref["waves"][i], S64, c) for i in (4, 32))
    wav = _np(eng.griffin_lim(fwd, [S32], 32, 0.99, None, [ang])[0])
    assert np.all(np.isfinite(wav))
    sc_eng = ir.spectral_convergence(wav.astype(np.float64), S64, c)
    print(f"GL-SC fft {sc.mel_id(c)} engine {sc_eng:.4f} restatement_4 {sc4:.4f} restatement_32 {sc32:.4f}")
    assert sc_eng <= sc32 + 0.25 * (sc4 - sc32)
    # n_iter = 0 is pk_istft_run of S * angles on the FFT path, bit for bit
    spec = np.concatenate([S32 * ang[:, :nb], S32 * ang[:, nb:]], axis=1)
    assert np.array_equal(_np(eng.griffin_lim(fwd, [S32], 0, 0.99, None, [ang])[0]), _np(eng.run([spec])[0]))
    # the seeded first iterate does not depend on the transform
    eng.griffin_lim(fwd, [S32], 0, 0.99, [11])
    first = _tap(eng, 1, F, nb)
    dense = _inv(c, "dense")
    dense.griffin_lim(_fwd(c, "dense"), [S32], 0, 0.99, [11])
    assert np.array_equal(first, _tap(dense, 1, F, nb)) and first.any()


# ------------------------------------------------------------------------------------------------ 8. surface
def test_refusals():
    from parakeet_amd import _capi
    from parakeet_amd.audio import ISTFT, STFT, AudioProcessor, LogMelFBank
    for n_fft, hop in ((400, 160), (48, 12)):
        for make in (lambda: STFT(n_fft, hop, transform="fft"), lambda: ISTFT(n_fft, hop, transform="fft"),
                     lambda: AudioProcessor(16000, n_fft, n_fft, hop, n_mels=10, transform="fft"),
                     lambda: LogMelFBank(16000, n_fft, hop, n_mels=10, transform="fft").get_log_mel_fbank(
                         np.zeros(4000, np.float32))):
            with pytest.raises(NotImplementedError, match="power of two from 32 to 4096"):
                make()
    with pytest.raises(ValueError, match="transform"):
        STFT(1024, 256, transform="radix")
    c = ir.GL_CFGS[1]
    fwd, inv = _fwd(c), _inv(c)
    lib = fwd.ctx.lib
    assert lib.pk_mel_set_transform(fwd.h, 7) == -1 and b"transform" in lib.pk_last_error()        # PK_EINVAL
    assert lib.pk_istft_set_transform(inv.h, -1) == -1
    S = np.ones((12, 33), np.float32)
    with pytest.raises(ValueError, match="transform"):                     # handles on different transforms
        inv.griffin_lim(_fwd(c, "dense"), [S], 1, 0.5)
    with pytest.raises(ValueError, match="transform"):
        _inv(c, "dense").griffin_lim(fwd, [S], 1, 0.5)
    assert _np(inv.griffin_lim(fwd, [S], 1, 0.5)[0]).shape == (16 * 11,)   # the handles still work, on their transform
    x = torch.zeros(8, 48)
    with pytest.raises(NotImplementedError, match="power of two from 32 to 4096"):
        from parakeet_amd import audio
        audio.rfft(x)
    assert _capi.PK_TRANSFORM == {"dense": 0, "fft": 1}


def test_default_is_the_dense_transform():
    from parakeet_amd.audio import STFT
    x = sc.mel_batch(sc.MEL_CFGS[0])[3][None, :3000]
    a, b, f = STFT(1024, 256), STFT(1024, 256, transform="dense"), STFT(1024, 256, transform="fft")
    for p, q in zip(a(x), b(x)):
        assert np.array_equal(_np(p), _np(q))
    assert np.array_equal(_np(a.magnitude(x)), _np(b.magnitude(x))) and np.array_equal(_np(a.power(x)), _np(b.power(x)))
    assert not np.array_equal(_np(a(x)[0]), _np(f(x)[0]))                  # and "fft" is another computation


def test_python_surface_on_the_fft_path(tmp_path):
    from parakeet_amd.audio import ISTFT, STFT, AudioProcessor, GriffinLim, LogMagnitude, LogMelFBank, _Engine
    c = sc.MEL_CFGS[0]
    ap = AudioProcessor(22050, 1024, 1024, 256, n_mels=80, fmin=0, fmax=8000, transform="fft")
    x = sc.mel_batch(c)[3][:3000]
    D = ap.stft(x)
    re, im = STFT(1024, 256, 1024, "hann", transform="fft")(x[None])
    assert D.dtype == np.complex64 and D.shape == (513, 1 + len(x) // 256)
    assert np.array_equal(D, (_np(re[0]) + 1j * _np(im[0])).astype(np.complex64))
    y = ap.istft(D)
    assert y.dtype == np.float32 and y.shape == (256 * (D.shape[1] - 1),)
    ref = rr.istft_fft(D.T.astype(np.complex128), c, err=rr.stft_fft(x, c)["bound"])
    assert fb.ratio(y, x[:y.size].astype(np.float64), ref["bound"] + 1e-12) <= 1.0
    assert np.array_equal(_np(ISTFT(1024, 256, 1024, "hann", transform="fft")(re, im)[0]), y)

    sig = ir.gl_signal(ir.GL_CFGS[0])[:11 * 256]
    logmel = LogMagnitude().transform(ap.mel_spectrogram(sig)).astype(np.float32)
    voc = GriffinLim(ap, LogMagnitude(), n_iter=4, momentum=0.99)
    w = voc.infer(logmel)
    assert w.shape == (256 * 11,) and w.dtype == np.float32 and np.all(np.isfinite(w))
    assert np.array_equal(w, ap.griffin_lim(ap.mel_to_linear(np.exp(logmel)), n_iter=4, momentum=0.99, seed=0))
    rag = voc.infer_batch([logmel[:, :9], logmel], seeds=[5, 0])
    assert rag[0].shape == (256 * 8,) and np.array_equal(rag[1], w)

    fbank = LogMelFBank(22050, 1024, 256, n_mels=80, fmin=80, fmax=7600, transform="fft")
    got = _np(fbank.get_log_mel_fbank(x))
    same = _Engine(1024, 256, 1024, "hann", True, False, fbank.mel_filter, 10, transform="fft")
    assert got.shape == (1 + len(x) // 256, 80) and np.all(np.isfinite(got)) and np.array_equal(got, _np(same.run([x], 2)[0]))

    # the example script: two 40-frame mels, 4 iterations
    long_sig = np.concatenate([ir.gl_signal(ir.GL_CFGS[0], s) for s in range(4)])[:39 * 256]
    mel = np.log(np.maximum(ap.mel_spectrogram(long_sig), 1e-5)).T.astype(np.float32)
    assert mel.shape == (40, 80)
    src, dst = tmp_path / "mels", tmp_path / "wavs"
    src.mkdir()
    np.save(src / "a_gta.npy", mel)
    np.save(src / "b_gta.npy", mel[::-1].copy())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "synthesize_griffin_lim.py"), "--input-dir", str(src),
                        "--output-dir", str(dst), "--n-iter", "4", "--transform", "fft"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("a_gta", "b_gta"):
        with wave.open(str(dst / f"{name}.wav"), "rb") as wv:
            assert wv.getframerate() == 22050 and wv.getnchannels() == 1 and wv.getnframes() == 256 * 39
            assert np.frombuffer(wv.readframes(wv.getnframes()), "<i2").any()
