"""The radix FFT of csrc/rfft.hip restated in numpy, and the error bound derived from its pass structure (a plain module,
not a conftest; shared by tests/test_rfft_cpu.py and tests/test_rfft_gpu.py).

The plan (csrc/pk_rfft.h): a real transform of n points is a complex transform of M = n/2 points z[m] = x[2m] + i x[2m+1],
floor(log2(M) / 2) radix-4 Stockham passes, one radix-2 pass where log2(M) is odd, and a split pass; twiddles T[t] =
exp(-2 pi i t / n) from a table computed in fp64 and rounded once to fp32.  ``rfft_f32`` / ``irfft_f32`` evaluate exactly
that structure in float32 (numpy rounds every operation; the device may fuse a product into the following addition, which
only removes roundings) and carry the mutants the CPU tests must reject.

THE BOUND.  u = 2^-24.  S = sum_n |x_n w_n| of a frame (w the window, 1 without).  Write S(y) for the sum of |x_n w_n|
over the samples an intermediate value y depends on; |y| <= S(y) in every pass, because every output is a sum of inputs
times factors of modulus 1 and the inputs of one butterfly depend on disjoint samples.  Claim: after p passes every value
carries an error of modulus <= E_p u S(y).
  * window product: fl(x w), one rounding; the issue budgets TWO (a window prepared in fp64 and rounded):  E_0 = 2.
  * complex product with a table entry: the entry is off by <= u in modulus (each component rounded once), the product
    itself by <= sqrt(5) u |a| < 3 u |a| (Brent, Percival, Zimmermann 2007; fewer with fused multiply-adds): 4 u |a|.
  * radix-4 pass: three such products feed two levels of complex additions (the factor -i is exact); an addition is off
    by <= u |result| <= u S(result) and the first level's error passes through the second with gain 1:  C_R4 = 4 + 2 = 6.
    The inputs' own errors add up: sum_q E u S(v_q) = E u S(out).  So E_(p+1) = E_p + 6.
  * radix-2 pass: one product, one level of additions:  C_R2 = 4 + 1 = 5.
  After the passes every Z[k] carries <= E_Z u S, E_Z = 2 + 6 R4 + 5 R2, and |Z[k]| <= S.
  * split pass X[k] = (A + T[k] B) / 2, A = Z[k] + conj Z[M-k], B = -i (Z[k] - conj Z[M-k]).  Z[k] and Z[M-k] depend on the
    SAME samples, so moduli are bounded by 2 S here: A and B are off by u 2S each, the product by 4 u 2S, the last
    addition by u (|A| + |B|) <= 4 u S; halved (exact): (2 + 2 + 8 + 4) / 2 = 8 u S.  The incoming errors reach X[k] through
    the coefficients (1 - i T[k]) / 2 and (1 + i T[k]) / 2, whose moduli add up to at most sqrt(2).
  rfft:  |dX[k]| <= (sqrt(2) E_Z + 8) u S =: RFFT_C(n) u S.          n = 1024: R4 = 4, R2 = 1, E_Z = 31, RFFT_C = 51.9
  (a radix-2 plan at 5u per level, the issue's calibration, has (log2 n + 2) 5 = 60 there; dot_bound has 2 (n + 2) = 2052
  on |a|.|w| >= S / sqrt(2).)

  irfft.  A = |X_0| + |X_M| + 2 sum_(0<k<M) |X_k| (real parts alone at k = 0 and M); every output sample is at most A / n.
  * pre-pass Z[k] = (X[k] + conj X[M-k]) + i conj(T[k]) (X[k] - conj X[M-k]): with P_k = |X_k| + |X_(M-k)| the two sums are
    off by u P_k each, the product by 4 u P_k, the last addition by u 2 P_k: 8 u P_k, and |Z[k]| <= 2 P_k.
    sum_(k<M) P_k = A.
  * the passes on sum_k |Z[k]| <= 2 A:  (6 R4 + 5 R2) u 2A, plus the pre-pass errors with gain 1: 8 u A.
  * the scale 1/n is a power of two (exact); the window product rounds once: u A / n.
  irfft: |dx_m| <= (9 + 2 (6 R4 + 5 R2)) u A / n =: IRFFT_C(n) u A / n   (times |w_m| under a window).
"""
import numpy as np

import fp32_bounds as fb

SIZES = (32, 64, 128, 256, 512, 1024, 2048, 4096)
C_PRODUCT, C_R4, C_R2, C_WINDOW, C_SPLIT, C_PRE = 4.0, 6.0, 5.0, 2.0, 8.0, 8.0


def passes(n):
    """(radix-4 passes, radix-2 passes) of the M = n/2 point complex transform."""
    lm = int(np.log2(n)) - 1
    assert 2 ** (lm + 1) == n, n
    return lm // 2, lm & 1


def rfft_c(n):
    r4, r2 = passes(n)
    return np.sqrt(2.0) * (C_WINDOW + C_R4 * r4 + C_R2 * r2) + C_SPLIT


def irfft_c(n):
    r4, r2 = passes(n)
    return C_PRE + 1.0 + 2.0 * (C_R4 * r4 + C_R2 * r2)


def rfft_bound(absx, n):
    """absx (rows, n) = |x_n w_n| -> (rows, 1): the bound on the complex error of every bin of that row (hence on re and
    on im)."""
    absx = np.asarray(absx, np.float64)
    assert absx.shape[-1] == n
    return rfft_c(n) * fb.U * absx.sum(-1, keepdims=True)


def spec_weight(absspec, n):
    """A of the module docstring, (rows, 1): |X_0| + |X_M| + 2 sum |X_k|."""
    a = np.asarray(absspec, np.float64)
    assert a.shape[-1] == n // 2 + 1
    return a[..., :1] + a[..., -1:] + 2.0 * a[..., 1:-1].sum(-1, keepdims=True)


def irfft_bound(absspec, n):
    """absspec (rows, n/2 + 1) = |X_k| (|re X_k| at DC and Nyquist) -> (rows, 1): the bound on every output sample of the
    row; under a synthesis window multiply by |w_m|."""
    return irfft_c(n) * fb.U * spec_weight(absspec, n) / n


def absspec(X):
    """|X_k| with the real part alone at DC and Nyquist (their imaginary parts are not read)."""
    X = np.asarray(X)
    a = np.abs(X).astype(np.float64)
    a[..., 0] = np.abs(X[..., 0].real)
    a[..., -1] = np.abs(X[..., -1].real)
    return a


def reim(X):
    X = np.asarray(X)
    return np.ascontiguousarray(np.concatenate([X.real, X.imag], axis=-1), dtype=np.float32)


def cplx(rows):
    rows = np.asarray(rows)
    nb = rows.shape[-1] // 2
    return rows[..., :nb].astype(np.float64) + 1j * rows[..., nb:].astype(np.float64)


# ------------------------------------------------------------------------------------- the plan in float32 numpy
def table(n, swap=None):
    """T[t] = exp(-2 pi i t / n) as (cos, sin) float32 pairs, the four axis points exact; ``swap``: entry swap replaced by
    its neighbour swap + 1 (a mutant)."""
    t = np.arange(n, dtype=np.float64)
    ang = -2.0 * np.pi * t / n
    T = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    q = n // 4
    T[0], T[q], T[2 * q], T[3 * q] = (1, 0), (0, -1), (-1, 0), (0, 1)
    T = T.astype(np.float32)
    if swap is not None:
        T[swap] = T[swap + 1]
    return T


def _mul(a, w):
    """float32 complex product as four products and two additions; a (..., 2), w (..., 2)"""
    return np.stack([a[..., 0] * w[..., 0] - a[..., 1] * w[..., 1], a[..., 0] * w[..., 1] + a[..., 1] * w[..., 0]], axis=-1)


def _mi(a):
    """-i a"""
    return np.stack([a[..., 1], -a[..., 0]], axis=-1)


def _conj(a):
    return np.stack([a[..., 0], -a[..., 1]], axis=-1)


def _passes_f32(z, n, T):
    """z (rows, M, 2) float32 -> its M-point DFT by the kernel's passes."""
    M = n // 2
    r4, r2 = passes(n)
    a = z
    for p in range(r4):
        Ns, Q = 4 ** p, M // 4
        j = np.arange(Q)
        k = j % Ns
        s = k * (n // (4 * Ns))
        v0 = a[:, j]
        v1 = _mul(a[:, j + Q], T[s])
        v2 = _mul(a[:, j + 2 * Q], T[2 * s])
        v3 = _mul(a[:, j + 3 * Q], T[3 * s])
        b0, b1, b2, b3 = v0 + v2, v0 - v2, v1 + v3, _mi(v1 - v3)
        j0 = (j - k) * 4 + k
        out = np.empty_like(a)
        out[:, j0], out[:, j0 + Ns], out[:, j0 + 2 * Ns], out[:, j0 + 3 * Ns] = b0 + b2, b1 + b3, b0 - b2, b1 - b3
        a = out
    if r2:
        H = M // 2
        j = np.arange(H)
        v0, v1 = a[:, j], _mul(a[:, j + H], T[2 * j])
        a = np.concatenate([v0 + v1, v0 - v1], axis=1)
    assert a.dtype == np.float32
    return a


def rfft_f32(x, window=None, mutant=None):
    """x (rows, n) -> (rows, n + 2) re | im float32, by the plan.  Mutants: "twiddle" (table entry n/8 + 1 replaced by its
    neighbour), "noconj" (the split pass without its conjugate), "nonyquist" (bin n/2 left at zero)."""
    x = np.asarray(x, np.float32)
    rows, n = x.shape
    M = n // 2
    T = table(n, swap=n // 8 + 1 if mutant == "twiddle" else None)
    if window is not None:
        x = x * np.asarray(window, np.float32)
    Z = _passes_f32(np.ascontiguousarray(x.reshape(rows, M, 2)), n, T)
    k = np.arange(M + 1)
    zk, zc = Z[:, k % M], Z[:, (M - k) % M]
    if mutant != "noconj":
        zc = _conj(zc)
    A, B = zk + zc, _mi(zk - zc)
    X = np.float32(0.5) * (A + _mul(B, T[k]))
    if mutant == "nonyquist":
        X[:, M] = 0
    return np.concatenate([X[..., 0], X[..., 1]], axis=1)


def irfft_f32(spec, window=None, mutant=None):
    """spec (rows, n + 2) re | im -> (rows, n) float32, by the plan.  Mutant "pair1": factor 1 instead of 2 on the bins that
    stand for a conjugate pair (an inverse that forgets the mirrored half)."""
    spec = np.asarray(spec, np.float32)
    rows, n = spec.shape[0], spec.shape[1] - 2
    M = n // 2
    T = table(n)
    X = np.stack([spec[:, :M + 1], spec[:, M + 1:]], axis=-1).copy()
    X[:, 0, 1] = 0
    X[:, M, 1] = 0
    if mutant == "pair1":
        X[:, 1:M] *= np.float32(0.5)
    k = np.arange(M)
    xk, xc = X[:, k], _conj(X[:, M - k])
    A = xk + xc
    Cc = _mul(xk - xc, _conj(T[k]))
    Zc = np.stack([A[..., 0] - Cc[..., 1], -(A[..., 1] + Cc[..., 0])], axis=-1)      # conj(A + i C)
    z = _passes_f32(Zc, n, T)
    y = np.stack([z[..., 0], -z[..., 1]], axis=-1) * np.float32(1.0 / n)
    y = y.reshape(rows, n)
    if window is not None:
        y = y * np.asarray(window, np.float32)
    assert y.dtype == np.float32
    return y


# ------------------------------------------------------------------------------------- inputs of tests 1 and 2
def row_inputs(n, rows, seed=0):
    """{name: (rows, n) float32}: gaussian, silence, +-1 alternating (all energy at Nyquist), an impulse at n - 1 (every bin
    has modulus 1), one sample 1e4 times louder than the rest."""
    r = np.random.default_rng([n, rows, seed])
    g = r.normal(0.0, 1.0, (rows, n)).astype(np.float32)
    alt = np.tile(np.where(np.arange(n) % 2 == 0, 1.0, -1.0), (rows, 1)).astype(np.float32)
    imp = np.zeros((rows, n), np.float32)
    imp[:, n - 1] = 1.0
    loud = (1e-2 * r.normal(0.0, 1.0, (rows, n))).astype(np.float32)
    loud[np.arange(rows), r.integers(0, n, rows)] = 100.0
    return {"gaussian": g, "silence": np.zeros((rows, n), np.float32), "nyquist": alt, "impulse": imp, "loud": loud}


def tile_row_counts(T):
    return sorted({1, max(1, T - 1), T, T + 1})


# ------------------------------------------------------------------------------------- STFT / ISTFT on the FFT path
def fft_cfgs():
    """The configurations of the FFT path's sweeps: the power-of-two entries of sweep_cases.MEL_CFGS, the small
    Griffin-Lim configuration and one at the smallest transform."""
    import sweep_cases as sc
    m = sc.MEL_CFGS
    return [m[0], m[1], m[4], m[5], sc.MelCfg(16000, 64, 16, 64, True, 10, None), sc.MelCfg(16000, 32, 8, 32, True, 10, None)]


def stft_fft(x, c, x_err=None):
    """fp64 STFT of one utterance as the FFT path computes it -> dict(spec (frames, n_bin) complex, bound (frames, 1)):
    rfft_bound of |frame * window|, plus a sample error ``x_err`` passed through the transform (a bin moves by at most
    sum_n |e_n w_n|)."""
    import istft_ref as ir
    win = ir.window64(c)
    x = np.asarray(x, np.float64)
    e = np.zeros_like(x) if x_err is None else np.asarray(x_err, np.float64)
    N = c.n_fft
    if c.center:
        x, e = np.pad(x, (N // 2, N // 2), mode="reflect"), np.pad(e, (N // 2, N // 2), mode="reflect")
    F = 0 if len(x) < N else 1 + (len(x) - N) // c.hop
    if F == 0:
        return dict(spec=np.zeros((0, 1 + N // 2), np.complex128), bound=np.zeros((0, 1)))
    A = np.stack([x[f * c.hop:f * c.hop + N] for f in range(F)]) * win
    E = np.stack([e[f * c.hop:f * c.hop + N] for f in range(F)]) * np.abs(win)
    return dict(spec=np.fft.rfft(A, axis=1), bound=rfft_bound(np.abs(A), N) + E.sum(1, keepdims=True))


def istft_fft(D, c, err=None):
    """istft_ref.istft's result and bound with the per-frame dot_bound replaced by irfft_bound * |window|.  ``err``
    (frames, n_bin) or (frames, 1): a bound on the complex error of each bin of D, passed through the linear inverse
    (a sample moves by at most (e_0 + e_M + 2 sum e_k) / n)."""
    import istft_ref as ir
    win = ir.window64(c)
    D = np.asarray(D, np.complex128)
    F, nb = D.shape
    N = c.n_fft
    rows = np.fft.irfft(D, n=N, axis=1) * win
    raw = ir.overlap_add(rows, c)
    env = ir.overlap_add(np.broadcast_to(win * win, (F, N)).copy(), c)
    nz = env > ir.FLT_MIN
    wav = np.where(nz, raw / np.where(nz, env, 1.0), raw)
    per_frame = irfft_bound(absspec(D), N)
    if err is not None:
        per_frame = per_frame + spec_weight(np.broadcast_to(np.asarray(err, np.float64), (F, nb)), N) / N
    nf = ir.overlap_add(np.ones((F, N)), c)
    num = ir.overlap_add(per_frame * np.abs(win), c) + (nf + 2.0) * fb.U * ir.overlap_add(np.abs(rows), c)
    bound = np.where(nz, num / np.where(nz, env, 1.0) + (nf + 2.0) * fb.U * np.abs(wav), num)
    return dict(wav=ir.trim(wav, c), bound=ir.trim(bound, c), env=ir.trim(env, c), raw=ir.trim(raw, c))
