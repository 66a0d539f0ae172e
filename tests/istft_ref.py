"""fp64 restatement of the inverse STFT and of fast Griffin-Lim, with a derived error bound for the inverse (a plain module,
not a conftest; shared by tests/test_istft_cpu.py and tests/test_istft_gpu.py).

Semantics (librosa 0.8 ``istft``, which is all parakeet/audio/audio.py:86-93 calls): every frame is
``irfft(D[:, f], n_fft) * window`` (the imaginary parts of DC and Nyquist are ignored, as numpy.fft.irfft does), frames are
overlap-added at stride hop, every sample is divided by the overlap-added ``window ** 2`` wherever that envelope exceeds
FLT_MIN and left undivided elsewhere, and with ``center`` n_fft/2 samples are cut from both ends.  ``griffin_lim`` is
librosa's ``griffinlim`` (Perraudin, Balazs, Sondergaard 2013): ``angles = rebuilt - momentum / (1 + momentum) * previous;
angles /= |angles| + 1e-16``.

Spectra are time-major here, (frames, n_bin) complex, like the C ABI's rows.

The bound.  The engine computes a frame as a K = 2 * n_bin term dot product of the frame's re | im row with a column of the
synthesis basis (irfft and window folded, prepared in fp64, stored as fp32), then adds up the nf frames that overlap a sample
and divides by the envelope.  Per sample
    bound = (sum_f dot_bound(|spec_f| . |basis[:, n - f hop]|, K) + (nf + 2) u sum_f |contribution_f|) / envelope
          + (nf + 2) u |result|
The first term is fp32_bounds.dot_bound per frame; the second covers the nf - 1 additions of the overlap-add with spare; the
last is the divide: the fp32 envelope is a sum of nf squares (one rounding each, nf - 1 additions: nf u relative), the
division itself rounds once (u), one spare.  Where the envelope is at or below FLT_MIN nothing is divided and the bound is
the bracket alone.
"""
import numpy as np

import fp32_bounds as fb
import sweep_cases as sc

FLT_MIN = float(np.finfo(np.float32).tiny)


def window64(c):
    return sc.window_f32(c).astype(np.float64)


def stft(x, c, win=None):
    """(T,) -> (frames, n_bin) complex128: reflect pad (center), frames at stride hop, rfft of frame * window."""
    win = window64(c) if win is None else np.asarray(win, np.float64)
    x = np.asarray(x, np.float64)
    N = c.n_fft
    if c.center:
        x = np.pad(x, (N // 2, N // 2), mode="reflect")
    F = 0 if len(x) < N else 1 + (len(x) - N) // c.hop
    if F == 0:
        return np.zeros((0, 1 + N // 2), np.complex128)
    A = np.stack([x[f * c.hop:f * c.hop + N] for f in range(F)])
    return np.fft.rfft(A * win, axis=1)


def num_samples(c, frames):
    return c.hop * (frames - 1) + (0 if c.center else c.n_fft)


def synthesis_basis(c, win=None, interior=2.0):
    """[re(k) | im(k)] x n_fft in fp64: x[n] = sum_k re X_k B[k, n] + im X_k B[n_bin + k, n].  ``interior`` is the factor on
    the bins that stand for a conjugate pair (2; a mutant passes 1)."""
    win = window64(c) if win is None else np.asarray(win, np.float64)
    N, nb = c.n_fft, 1 + c.n_fft // 2
    k, n = np.arange(nb)[:, None], np.arange(N)[None, :]
    ang = 2.0 * np.pi * ((k * n) % N) / N
    s = np.full((nb, 1), interior / N)
    s[0] = s[-1] = 1.0 / N
    B = np.concatenate([s * np.cos(ang), -s * np.sin(ang)], axis=0) * win
    B[nb] = 0.0
    B[2 * nb - 1] = 0.0
    return B


def reim(D):
    D = np.asarray(D)
    return np.concatenate([D.real, D.imag], axis=1)


def overlap_add(rows, c, drop_frame=None):
    """(frames, n_fft) -> (n_fft + hop * (frames - 1),) ; ``drop_frame`` leaves one frame out (a mutant)."""
    F, N = rows.shape
    y = np.zeros(N + c.hop * (F - 1), dtype=rows.dtype)
    for f in range(F):
        if f != drop_frame:
            y[f * c.hop:f * c.hop + N] += rows[f]
    return y


def trim(y, c):
    return y[c.n_fft // 2:len(y) - c.n_fft // 2] if c.center else y


def istft(D, c, win=None, with_bound=False, err=None, basis=None):
    """D (frames, n_bin) complex -> wav (fp64); with_bound: dict(wav, bound, env, nf, raw) where ``raw`` is the undivided
    overlap-add, ``env`` the envelope (all trimmed alike) and ``bound`` the module docstring's.  ``err`` (frames, n_bin):
    an absolute error bound on each complex bin of D, propagated through the linear inverse into the bound
    (|d re| and |d im| <= err)."""
    win = window64(c) if win is None else np.asarray(win, np.float64)
    D = np.asarray(D, np.complex128)
    F, nb = D.shape
    N = c.n_fft
    rows = np.fft.irfft(D, n=N, axis=1) * win
    raw = overlap_add(rows, c)
    env = overlap_add(np.broadcast_to(win * win, (F, N)).copy(), c)
    nz = env > FLT_MIN
    wav = np.where(nz, raw / np.where(nz, env, 1.0), raw)
    if not with_bound:
        return trim(wav, c)
    B = synthesis_basis(c, win) if basis is None else basis
    A = np.abs(reim(D))
    absrows = A @ np.abs(B)
    nf = overlap_add(np.ones((F, N)), c)
    num = overlap_add(fb.dot_bound(absrows, 2 * nb), c) + (nf + 2.0) * fb.U * overlap_add(np.abs(rows), c)
    if err is not None:
        e = np.asarray(err, np.float64)
        num = num + overlap_add(np.concatenate([e, e], axis=1) @ np.abs(B), c)
    bound = np.where(nz, num / np.where(nz, env, 1.0) + (nf + 2.0) * fb.U * np.abs(wav), num)
    return dict(wav=trim(wav, c), bound=trim(bound, c), env=trim(env, c), nf=trim(nf, c), raw=trim(raw, c))


def istft_f32(D, c, win=None, drop_frame=None, env_short=False, interior=2.0):
    """A float32 numpy evaluation in the engine's order (basis product, overlap-add, envelope, divide), and its mutants."""
    win = window64(c) if win is None else np.asarray(win, np.float64)
    B = synthesis_basis(c, win, interior).astype(np.float32)
    rows = reim(D).astype(np.float32) @ B
    raw = overlap_add(rows, c, drop_frame)
    w2 = (win.astype(np.float32) ** 2).astype(np.float32)
    F = rows.shape[0]
    env = overlap_add(np.broadcast_to(w2, (F, c.n_fft)).copy(), c, drop_frame=F - 1 if env_short and F > 1 else None)
    nz = env > np.float32(FLT_MIN)
    return trim(np.where(nz, raw / np.where(nz, env, np.float32(1)), raw).astype(np.float32), c)


def stft_bound(x, c, win=None, x_err=None):
    """Bound on the engine's forward STFT of x as complex modulus per bin, (frames, n_bin): fp32_bounds.dot_bound of the
    two products (as sweep_cases.mel_reference), plus an absolute error ``x_err`` on the samples passed through |W|."""
    win = window64(c) if win is None else np.asarray(win, np.float64)
    x = np.asarray(x, np.float64)
    N, nb = c.n_fft, 1 + c.n_fft // 2
    e = np.zeros_like(x) if x_err is None else np.asarray(x_err, np.float64)
    if c.center:
        x, e = np.pad(x, (N // 2, N // 2), mode="reflect"), np.pad(e, (N // 2, N // 2), mode="reflect")
    F = 1 + (len(x) - N) // c.hop
    A = np.stack([np.abs(x[f * c.hop:f * c.hop + N]) for f in range(F)])
    E = np.stack([e[f * c.hop:f * c.hop + N] for f in range(F)])
    n, k = np.arange(N)[:, None], np.arange(nb)[None, :]
    ang = -2.0 * np.pi * ((n * k) % N) / N
    W = np.abs(np.concatenate([np.cos(ang) * win[:, None], np.sin(ang) * win[:, None]], axis=1))
    b = fb.dot_bound(A @ W, N) + E @ W
    return np.hypot(b[:, :nb], b[:, nb:])


def gl_update(rebuilt, previous, momentum):
    a = rebuilt - momentum / (1.0 + momentum) * previous
    return a / (np.abs(a) + 1e-16)


def griffin_lim(S, c, n_iter, momentum, angles, win=None, keep=()):
    """S (frames, n_bin) magnitudes, angles (frames, n_bin) complex initial phases -> dict(wav, rebuilt, angles, waves):
    ``rebuilt`` / ``angles`` after the last update, ``waves[i]`` = istft(S * angles) after i updates for i in ``keep``."""
    S = np.asarray(S, np.float64)
    angles = np.asarray(angles, np.complex128)
    rebuilt = np.zeros_like(angles)
    waves = {}
    for it in range(n_iter):
        if it in keep:
            waves[it] = istft(S * angles, c, win)
        previous = rebuilt
        rebuilt = stft(istft(S * angles, c, win), c, win)
        angles = gl_update(rebuilt, previous, momentum)
    wav = istft(S * angles, c, win)
    if n_iter in keep:
        waves[n_iter] = wav
    return dict(wav=wav, rebuilt=rebuilt, angles=angles, waves=waves)


def spectral_convergence(wav, S, c, win=None):
    """|| |stft(wav)| - S ||_F / || S ||_F with the fp64 STFT above."""
    return float(np.linalg.norm(np.abs(stft(wav, c, win)) - S) / np.linalg.norm(S))


def gl_signal(c, seed=0):
    """0.3 sin(2 pi 0.01 t) + 0.2 sin(2 pi 0.043 t + 1) + 0.05 N(0, 1), n_fft + 9 hop samples."""
    t = np.arange(c.n_fft + 9 * c.hop, dtype=np.float64)
    r = sc.rng_for("gl", c.n_fft, c.hop, seed)
    return 0.3 * np.sin(2 * np.pi * 0.01 * t) + 0.2 * np.sin(2 * np.pi * 0.043 * t + 1.0) + 0.05 * r.normal(size=t.size)


GL_CFGS = [sc.MelCfg(22050, 1024, 256, 1024, True, 80, None), sc.MelCfg(16000, 64, 16, 64, True, 10, None)]


def gl_problem(c):
    """-> S (frames, n_bin) fp64 magnitudes of the test signal, angles0 (frames, n_bin) complex unit-modulus phases."""
    S = np.abs(stft(gl_signal(c), c))
    r = np.random.default_rng(1234 + c.n_fft)
    return S, np.exp(2j * np.pi * r.random(S.shape))


def sweep_spectra(c):
    """The ragged batch of the inverse sweep: the fp64 STFTs of sweep_cases.mel_batch(c) (zero-frame utterances left out),
    a one-frame and a two-frame utterance, and a random complex spectrum that is the STFT of no signal, with non-zero
    imaginary DC and Nyquist.  Rounded to what the engine receives: complex64."""
    out = [stft(w, c) for w in sc.mel_batch(c)]
    out = [D for D in out if D.shape[0] > 0]
    r = sc.rng_for("istft", *c)
    nb = 1 + c.n_fft // 2
    long_one = out[-1]
    out.append(long_one[3:4].copy())
    out.append(long_one[5:7].copy())
    out.append(r.normal(0.2, 1.0, (5, nb)) + 1j * r.normal(-0.1, 1.0, (5, nb)))
    return [D.astype(np.complex64) for D in out]
