"""The radix FFT's plan and its derived bound on the CPU (tests/rfft_ref.py): the float32 numpy evaluation of the kernel's
pass structure stays under rfft_bound / irfft_bound, the bounds reject wrong transforms, and they are tighter than the
dense product's dot_bound for every size the kernel takes.  Nothing here runs the engine's kernels; the last test reads the
engine's size predicate and tile, which need the library but no GPU."""
import numpy as np
import pytest

import fp32_bounds as fb
import rfft_ref as rr


def _ref(x):
    return np.fft.rfft(x.astype(np.float64), axis=1)


def _fwd_ratio(got, x, n):
    want = _ref(x)
    b = rr.rfft_bound(np.abs(x.astype(np.float64)), n)
    return max(fb.ratio(got[:, :n // 2 + 1], want.real, b), fb.ratio(got[:, n // 2 + 1:], want.imag, b))


@pytest.mark.parametrize("n", rr.SIZES)
def test_plan_in_float32_is_inside_both_bounds(n):
    worst_f = worst_i = 0.0
    for name, x in rr.row_inputs(n, 3).items():
        got = rr.rfft_f32(x)
        worst_f = max(worst_f, _fwd_ratio(got, x, n))
        X = _ref(x).astype(np.complex64)
        want = np.fft.irfft(X.astype(np.complex128), n=n, axis=1)
        worst_i = max(worst_i, fb.ratio(rr.irfft_f32(rr.reim(X)), want, rr.irfft_bound(rr.absspec(X), n)))
        if name == "silence":
            assert not got.any()
        if name == "impulse":
            assert np.abs(np.abs(rr.cplx(got)) - 1.0).max() <= 64 * fb.U
    print(f"SWEEP-RATIO rfft_f32 n{n} forward {worst_f:.4g} inverse {worst_i:.4g}")
    assert worst_f <= 1.0 and worst_i <= 1.0


@pytest.mark.parametrize("n", rr.SIZES)
def test_window_and_ignored_imaginary_parts(n):
    r = np.random.default_rng(n)
    x = r.normal(0, 1, (2, n)).astype(np.float32)
    w = np.hanning(n + 1)[:n].astype(np.float32)
    xw = x.astype(np.float64) * w.astype(np.float64)
    want = np.fft.rfft(xw, axis=1)
    got = rr.rfft_f32(x, window=w)
    b = rr.rfft_bound(np.abs(xw), n)
    assert max(fb.ratio(got[:, :n // 2 + 1], want.real, b), fb.ratio(got[:, n // 2 + 1:], want.imag, b)) <= 1.0
    X = (r.normal(0, 1, (2, n // 2 + 1)) + 1j * r.normal(0, 1, (2, n // 2 + 1))).astype(np.complex64)
    rows = rr.reim(X)
    base = rr.irfft_f32(rows, window=w)
    rows[:, n // 2 + 1] = np.nan
    rows[:, -1] = np.nan
    assert np.array_equal(rr.irfft_f32(rows, window=w), base) and np.all(np.isfinite(base))
    want = np.fft.irfft(X.astype(np.complex128), n=n, axis=1) * w
    assert fb.ratio(base, want, rr.irfft_bound(rr.absspec(X), n) * np.abs(w.astype(np.float64))) <= 1.0


@pytest.mark.parametrize("n", rr.SIZES)
def test_mutants_are_rejected(n):
    ins = rr.row_inputs(n, 3)
    for m in ("twiddle", "noconj", "nonyquist"):
        assert max(_fwd_ratio(rr.rfft_f32(x, mutant=m), x, n) for x in ins.values()) > 1.0, m
    x = ins["gaussian"]
    X = _ref(x).astype(np.complex64)
    want = np.fft.irfft(X.astype(np.complex128), n=n, axis=1)
    assert fb.ratio(rr.irfft_f32(rr.reim(X), mutant="pair1"), want, rr.irfft_bound(rr.absspec(X), n)) > 1.0


@pytest.mark.parametrize("n", rr.SIZES)
def test_bound_is_below_the_dense_products(n):
    """fp32_bounds.dot_bound of the two dense products, as istft_ref.stft_bound and istft_ref.istft apply it (modulus of
    the re and im bounds forward, |re| |cos| + |im| |sin| inverse), against the FFT's bounds on random frames and spectra."""
    r = np.random.default_rng(n + 1)
    nb = n // 2 + 1
    x = np.abs(r.normal(0, 1, (4, n)))
    k, t = np.arange(nb)[None, :], np.arange(n)[:, None]
    ang = 2.0 * np.pi * ((t * k) % n) / n
    d = fb.dot_bound(x @ np.abs(np.concatenate([np.cos(ang), np.sin(ang)], axis=1)), n)
    dense = np.hypot(d[:, :nb], d[:, nb:])
    fwd = float((dense / rr.rfft_bound(x, n)).min())
    X = r.normal(0, 1, (4, nb)) + 1j * r.normal(0, 1, (4, nb))
    s = np.full((nb, 1), 2.0 / n)
    s[0] = s[-1] = 1.0 / n
    B = np.abs(np.concatenate([s * np.cos(ang.T), s * np.sin(ang.T)], axis=0))
    B[nb] = B[2 * nb - 1] = 0.0
    dense_inv = fb.dot_bound(np.abs(np.concatenate([X.real, X.imag], axis=1)) @ B, 2 * nb)
    inv = float((dense_inv / rr.irfft_bound(rr.absspec(X), n)).min())
    print(f"SWEEP-INFO rfft_bound n{n} constants forward {rr.rfft_c(n):.1f} inverse {rr.irfft_c(n):.1f} dense {2 * (n + 2)}; "
          f"smallest dense / fft bound forward {fwd:.1f} inverse {inv:.1f}")
    assert fwd > 1.0 and inv > 1.0


def test_engine_reports_the_sizes_and_tiles():
    from parakeet_amd import audio
    for n in (16, 31, 32, 48, 400, 1024, 4096, 8192):
        assert audio.rfft_supported(n) == (n in rr.SIZES), n
    for n in rr.SIZES:
        assert audio.rfft_tile_rows(n) == max(1, 2048 // n)
    with pytest.raises(NotImplementedError, match="power of two from 32 to 4096"):
        audio.rfft_tile_rows(400)
