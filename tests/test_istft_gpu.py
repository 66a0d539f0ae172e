"""Inverse STFT and Griffin-Lim on the engine (csrc/istft.hip) against the fp64 restatement of tests/istft_ref.py under its
derived bound: the sweep over sweep_cases.MEL_CFGS, the device round trip, batch invariance bit for bit, one Griffin-Lim step,
a whole Griffin-Lim run, the seeded phase stream, the Python surface and the refusals.  ``SWEEP-RATIO`` lines give error /
bound.

Griffin-Lim, whole run, first hardware run, SC_engine / SC_ref(4) / SC_ref(32): 0.1768 / 0.2228 / 0.1768 at
1024 / 256 and 0.2154 / 0.2800 / 0.2154 at 64 / 16.
"""
import ctypes as C
import functools
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import fp32_bounds as fb
import istft_ref as ir
import sweep_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.detach().cpu().numpy()


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _rows(D):
    return np.ascontiguousarray(ir.reim(D), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _inv(c, window="hann"):
    from parakeet_amd.audio import _InvEngine
    return _InvEngine(c.n_fft, c.hop, c.win, window, c.center)


@functools.lru_cache(maxsize=None)
def _fwd(c, window="hann"):
    from parakeet_amd.audio import _Engine
    return _Engine(c.n_fft, c.hop, c.win, window, c.center, False, None, 0)


def _run_host(eng, rows):
    from parakeet_amd import _capi
    frames = np.array([r.shape[0] for r in rows], dtype=np.int32)
    x = np.ascontiguousarray(np.concatenate(rows), dtype=np.float32)
    out = np.full(sum(eng.samples(f) for f in frames), np.nan, np.float32)
    _capi.check(eng.ctx.lib.pk_istft_run(eng.h, _capi.fptr(x), _i32(frames), len(rows), _capi.fptr(out), _capi.PK_HOST_IO))
    return out


def _tap(eng, what, frames, nb):
    from parakeet_amd import _capi
    out = np.empty((frames, 2 * nb), np.float32)
    _capi.check(eng.ctx.lib.pk_gl_debug_read(eng.h, what, _capi.fptr(out), out.size))
    return out


@functools.lru_cache(maxsize=None)
def _sweep(c):
    """The sweep's batch, run once per configuration: spectra, their rows, the device result per utterance."""
    specs = ir.sweep_spectra(c)
    rows = [_rows(D) for D in specs]
    got = [_np(o) for o in _inv(c).run(rows)]
    return specs, rows, got


# ------------------------------------------------------------------------------------------------ 1. sweep
@pytest.mark.parametrize("c", sc.MEL_CFGS, ids=sc.mel_id)
def test_istft_sweep(c):
    specs, rows, got = _sweep(c)
    eng = _inv(c)
    B = ir.synthesis_basis(c)
    assert {1, 2} <= {D.shape[0] for D in specs}
    worst, worst_raw = 0.0, 0.0
    for D, y in zip(specs, got):
        assert y.shape == (eng.samples(D.shape[0]),) == (ir.num_samples(c, D.shape[0]),)
        ref = ir.istft(D, c, with_bound=True, basis=B)
        divided = ref["env"] > ir.FLT_MIN
        worst = max(worst, fb.ratio(y, ref["wav"], ref["bound"], divided))
        # at or below FLT_MIN: the undivided sum, under the bound without the division
        worst_raw = max(worst_raw, fb.ratio(y, ref["raw"], ref["bound"], ~divided))
        if not c.center:
            assert not divided[0] and y[0] == 0.0        # the periodic hann window is 0 at sample 0: exactly 0
    print(f"SWEEP-RATIO istft {sc.mel_id(c)} divided {worst:.4g}")
    print(f"SWEEP-RATIO istft {sc.mel_id(c)} undivided {worst_raw:.4g}")
    assert worst <= 1.0 and worst_raw <= 1.0
    assert not got[1].any()                              # silence stays silence
    assert np.array_equal(_run_host(eng, rows), np.concatenate(got))      # PK_HOST_IO, bit for bit


# ------------------------------------------------------------------------------------------------ 2. round trip
@pytest.mark.parametrize("c", [c for c in sc.MEL_CFGS if c.center], ids=sc.mel_id)
def test_round_trip_on_the_device(c):
    """ISTFT(STFT(x)) against x over the hop * (frames - 1) samples returned.  The engine inverts ITS spectrum D' = D + e,
    |e| <= the forward bound: the inverse bound at D' plus e passed through the linear inverse is the limit (the exact
    inverse of the exact D is x itself, to the 1e-12 of test_istft_cpu)."""
    wavs = sc.mel_batch(c)
    spec = _fwd(c).run(wavs, 0)
    back = [_np(o) for o in _inv(c).run(spec)]
    B = ir.synthesis_basis(c)
    nb = 1 + c.n_fft // 2
    worst = 0.0
    for w, s, y in zip(wavs, spec, back):
        s = _np(s).astype(np.float64)
        ref = ir.istft(s[:, :nb] + 1j * s[:, nb:], c, with_bound=True, err=ir.stft_bound(w, c), basis=B)
        assert y.shape == (c.hop * (s.shape[0] - 1),)
        worst = max(worst, fb.ratio(y, w[:y.size].astype(np.float64), ref["bound"] + 1e-12))
    print(f"SWEEP-RATIO istft_round_trip {sc.mel_id(c)} {worst:.4g}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 3. batch invariance
@pytest.mark.parametrize("c", sc.MEL_CFGS, ids=sc.mel_id)
def test_batch_invariance_bit_for_bit(c):
    _, rows, got = _sweep(c)
    eng = _inv(c)
    for u, r in enumerate(rows):
        others = [x for v, x in enumerate(rows) if v != u][:3]
        assert np.array_equal(_np(eng.run([r])[0]), got[u]), ("alone", u)
        assert np.array_equal(_np(eng.run([r] + others)[0]), got[u]), ("first", u)
        assert np.array_equal(_np(eng.run(others + [r])[-1]), got[u]), ("last", u)


# ------------------------------------------------------------------------------------------------ 4. / 5. Griffin-Lim
@functools.lru_cache(maxsize=None)
def _gl_case(c):
    """S and the initial angles as the engine receives them (float32), and the restatement's run on exactly those."""
    S, a0 = ir.gl_problem(c)
    S32 = S.astype(np.float32)
    ang = _rows(a0)                                       # cos | sin, float32
    nb = S.shape[1]
    S64, a64 = S32.astype(np.float64), ang[:, :nb].astype(np.float64) + 1j * ang[:, nb:].astype(np.float64)
    return S32, ang, S64, a64


@pytest.mark.parametrize("c", ir.GL_CFGS, ids=sc.mel_id)
def test_griffin_lim_one_step(c):
    S32, ang, S64, a64 = _gl_case(c)
    F, nb = S32.shape
    eng, fwd = _inv(c), _fwd(c)
    ref = ir.griffin_lim(S64, c, 1, 0.99, a64)
    wav = _np(eng.griffin_lim(fwd, [S32], 1, 0.99, None, [ang])[0])
    rebuilt, iterate = _tap(eng, 0, F, nb), _tap(eng, 1, F, nb)
    # the returned waveform is the ISTFT of the tapped iterate S * angles
    assert np.array_equal(wav, _np(eng.run([iterate])[0]))

    # step 1: the rebuilt spectrum.  x0 = istft(S * angles0) carries the inverse bound; the forward transform adds its own
    # and passes the former through |W|
    x0 = ir.istft(S64 * a64, c, with_bound=True)
    b_reb = ir.stft_bound(x0["wav"], c, x_err=x0["bound"])
    err = np.abs((rebuilt[:, :nb].astype(np.float64) + 1j * rebuilt[:, nb:]) - ref["rebuilt"])
    r1 = float((err / b_reb).max())
    print(f"SWEEP-RATIO gl_one_step {sc.mel_id(c)} rebuilt {r1:.4g}")
    assert r1 <= 1.0

    # step 2 from shared angles: where |rebuilt| is tiny the phase is ill-conditioned; both sides get the restatement's
    # angles there.  Elsewhere the engine's angles are off by at most delta = bound(rebuilt) / |rebuilt|: S * delta per bin.
    mag = np.abs(ref["rebuilt"])
    excl = mag < 1e-3 * mag.max()
    share = excl.mean()
    print(f"SWEEP-INFO gl_one_step {sc.mel_id(c)} excluded_share {share:.4f}")
    assert share <= 0.05
    want_spec = S64 * ref["angles"]
    X = iterate[:, :nb].astype(np.complex128) + 1j * iterate[:, nb:]
    X[excl] = want_spec[excl]
    X = X.astype(np.complex64)
    e = np.where(excl, 2.0 * fb.U * S64, S64 * b_reb / np.where(excl, 1.0, mag))
    lim = ir.istft(want_spec, c, with_bound=True, err=e)
    r2 = fb.ratio(_np(eng.run([_rows(X)])[0]), lim["wav"], lim["bound"])
    print(f"SWEEP-RATIO gl_one_step {sc.mel_id(c)} wav {r2:.4g}")
    assert r2 <= 1.0
    assert wav.shape == lim["wav"].shape and np.all(np.isfinite(wav))


@pytest.mark.parametrize("c", ir.GL_CFGS, ids=sc.mel_id)
def test_griffin_lim_whole_run(c):
    """fp32 and fp64 trajectories may drift apart, so spectral convergence is compared, with the restatement's fp64 STFT:
    the engine keeps at least three quarters of what the restatement gains between iterations 4 and 32."""
    S32, ang, S64, a64 = _gl_case(c)
    eng, fwd = _inv(c), _fwd(c)
    ref = ir.griffin_lim(S64, c, 32, 0.99, a64, keep=(4, 32))
    sc4, sc32 = (ir.spectral_convergence(ref["waves"][i], S64, c) for i in (4, 32))
    wav = _np(eng.griffin_lim(fwd, [S32], 32, 0.99, None, [ang])[0])
    assert np.all(np.isfinite(wav))
    sc_eng = ir.spectral_convergence(wav.astype(np.float64), S64, c)
    print(f"GL-SC {sc.mel_id(c)} engine {sc_eng:.4f} restatement_4 {sc4:.4f} restatement_32 {sc32:.4f}")
    assert sc_eng <= sc32 + 0.25 * (sc4 - sc32)
    # n_iter = 0 is pk_istft_run of S * angles, bit for bit
    nb = S32.shape[1]
    spec = np.concatenate([S32 * ang[:, :nb], S32 * ang[:, nb:]], axis=1)
    assert np.array_equal(_np(eng.griffin_lim(fwd, [S32], 0, 0.99, None, [ang])[0]), _np(eng.run([spec])[0]))


# ------------------------------------------------------------------------------------------------ 6. seeds
def test_seeded_phases():
    from oracle import philox_ref
    c = ir.GL_CFGS[1]
    S32 = _gl_case(c)[0]
    F, nb = S32.shape
    eng, fwd = _inv(c), _fwd(c)
    other = np.ascontiguousarray(S32[:7] * 0.5)

    def run(mags, seeds, n_iter=3):
        return [_np(o) for o in eng.griffin_lim(fwd, mags, n_iter, 0.99, seeds)]

    a = run([S32], [7])[0]
    assert np.array_equal(a, run([S32], [7])[0])                          # the same seed twice
    assert np.array_equal(a, run([other, S32], [3, 7])[1])                # alone and inside a ragged batch
    assert np.array_equal(a, run([S32, other], [7, 3])[0])
    assert not np.array_equal(a, run([S32], [8])[0])                      # two seeds differ
    assert np.all(np.isfinite(a))

    # the drawn phases, read back as the iterate of an n_iter = 0 run against S = 1: unit modulus, and the documented
    # stream -- word (bin & 3) of the Philox block (frame, bin >> 2, 0, "GLPH") under the utterance's seed
    ones = np.ones((F, nb), np.float32)
    seed = (5 << 32) + 11
    run([np.ones((2, nb), np.float32), ones], [1, seed], n_iter=0)
    it = _tap(eng, 1, 2 + F, nb)[2:]
    ph = it[:, :nb].astype(np.float64) + 1j * it[:, nb:]
    assert np.abs(np.abs(ph[:, 1:-1]) - 1.0).max() <= 4.0 * fb.U
    f, k = np.meshgrid(np.arange(F), np.arange(nb), indexing="ij")
    ctr = np.stack([f, k >> 2, np.zeros_like(f), np.full_like(f, 0x474C5048)], axis=-1)
    words = philox_ref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    w = np.take_along_axis(words, (k & 3)[..., None], axis=-1)[..., 0]
    u = np.float32(w).astype(np.float64) * 2.0 ** -32
    want = np.exp(2j * np.pi * u)
    want[:, [0, -1]] = want[:, [0, -1]].real                              # im(DC), im(Nyquist) are not part of a spectrum
    assert np.abs(ph - want).max() <= 8.0 * fb.U                          # sincospif: a few ulp of values <= 1


# ------------------------------------------------------------------------------------------------ 7. Python surface
def _processor():
    from parakeet_amd.audio import AudioProcessor
    return AudioProcessor(22050, 1024, 1024, 256, n_mels=80, fmin=0, fmax=8000)


def test_audio_processor_stft_istft():
    from parakeet_amd.audio import ISTFT, STFT
    ap = _processor()
    c = sc.MEL_CFGS[0]
    x = sc.mel_batch(c)[3][:3000]
    D = ap.stft(x)
    re, im = STFT(1024, 256, 1024, "hann")(x[None])
    assert D.dtype == np.complex64 and D.shape == (513, 1 + len(x) // 256)
    assert np.array_equal(D, (_np(re[0]) + 1j * _np(im[0])).astype(np.complex64))
    y = ap.istft(D)
    assert y.dtype == np.float32 and y.shape == (256 * (D.shape[1] - 1),)
    ref = ir.istft(D.T.astype(np.complex128), c, with_bound=True, err=ir.stft_bound(x, c))
    assert fb.ratio(y, x[:y.size].astype(np.float64), ref["bound"] + 1e-12) <= 1.0
    inv = ISTFT(1024, 256, 1024, "hann")
    assert np.array_equal(_np(inv(re, im)[0]), y)
    assert np.array_equal(_np(inv.inverse_batch([torch.cat([re[0], im[0]], 0).transpose(0, 1)])[0]), y)


def test_mel_to_linear():
    ap = _processor()
    mel = np.abs(sc.rng_for("m2l").normal(0.5, 1.0, (80, 37))).astype(np.float32)
    got = ap.mel_to_linear(mel)
    P, M = ap.inv_mel_filter.astype(np.float64), mel.astype(np.float64)
    lin = P @ M
    bound = fb.dot_bound(np.abs(P) @ np.abs(M), 80)
    want = np.maximum(1e-10, lin)
    assert got.shape == (513, 37) and got.dtype == np.float32
    # max(., 1e-10) is 1-Lipschitz: the product's bound carries over, plus the rounding of the floor constant
    assert fb.ratio(got, want, bound + fb.U * 1e-10) <= 1.0
    assert got.min() >= np.float32(1e-10) and (lin < 0).any()


def test_griffin_lim_vocoder():
    from parakeet_amd.audio import GriffinLim, LogMagnitude
    ap = _processor()
    x = ir.gl_signal(ir.GL_CFGS[0])[:11 * 256]
    logmel = LogMagnitude().transform(ap.mel_spectrogram(x)).astype(np.float32)
    assert logmel.shape == (80, 12)
    voc = GriffinLim(ap, LogMagnitude(), n_iter=4, momentum=0.99)
    y = voc.infer(logmel)
    assert y.shape == (256 * 11,) and y.dtype == np.float32 and np.all(np.isfinite(y))
    # the three calls by hand give the same bytes: the same rows go through the same kernels
    assert np.array_equal(y, ap.griffin_lim(ap.mel_to_linear(np.exp(logmel)), n_iter=4, momentum=0.99, seed=0))
    sharp = GriffinLim(ap, LogMagnitude(), n_iter=4, momentum=0.99, power=1.2).infer(logmel)
    assert sharp.shape == y.shape and np.all(np.isfinite(sharp)) and not np.array_equal(sharp, y)
    two = voc.infer(np.stack([logmel, logmel]))
    assert two.shape == (2, 256 * 11) and np.array_equal(two[0], y) and np.array_equal(two[1], y)
    rag = voc.infer_batch([logmel[:, :9], logmel], seeds=[5, 0])
    assert rag[0].shape == (256 * 8,) and np.array_equal(rag[1], y)


def test_example_writes_wav_files(tmp_path):
    ap = _processor()
    x = ir.gl_signal(ir.GL_CFGS[0])
    mel = np.log(np.maximum(ap.mel_spectrogram(x), 1e-5)).T.astype(np.float32)      # (frames, n_mels) like the GTA scripts
    src, dst = tmp_path / "mels", tmp_path / "wavs"
    src.mkdir()
    np.save(src / "a_gta.npy", mel)
    np.save(src / "b_gta.npy", mel[:9])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "synthesize_griffin_lim.py"), "--input-dir", str(src),
                        "--output-dir", str(dst), "--n-iter", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name, frames in (("a_gta", mel.shape[0]), ("b_gta", 9)):
        with wave.open(str(dst / f"{name}.wav"), "rb") as w:
            assert w.getframerate() == 22050 and w.getnchannels() == 1 and w.getnframes() == 256 * (frames - 1)
            assert np.frombuffer(w.readframes(w.getnframes()), "<i2").any()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    from parakeet_amd.audio import _InvEngine
    c = sc.MEL_CFGS[0]
    eng, fwd = _inv(c), _fwd(c)
    nb = 513
    with pytest.raises(AssertionError, match="rows"):                      # wrong column count
        eng.run([np.zeros((3, 2 * nb - 1), np.float32)])
    with pytest.raises(ValueError, match="at least 1"):                    # frames[b] = 0
        eng.run([np.zeros((3, 2 * nb), np.float32), np.zeros((0, 2 * nb), np.float32)])
    with pytest.raises(NotImplementedError, match="multiple of 16"):       # n_fft % 16 != 0
        _InvEngine(1000, 200, 1000, "hann", True)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        _InvEngine(1024, 250, 1024, "hann", True)
    S = np.ones((6, nb), np.float32)
    with pytest.raises(ValueError, match="does not match"):                # mismatched handles
        eng.griffin_lim(_fwd(sc.MEL_CFGS[5]), [S], 1, 0.5)
    with pytest.raises(ValueError, match="n_iter"):
        eng.griffin_lim(fwd, [S], -1, 0.5)
    for m in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            eng.griffin_lim(fwd, [S], 1, m)
    with pytest.raises(ValueError, match="too short"):                     # hop * (frames - 1) <= n_fft / 2
        eng.griffin_lim(fwd, [S[:3]], 1, 0.5)
    assert _np(eng.griffin_lim(fwd, [S], 1, 0.5)[0]).shape == (256 * 5,)   # and the handle still works
