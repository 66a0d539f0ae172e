"""Derived error bounds for comparing the engine's fp32 kernels with fp64 references (a plain module, not a conftest).

Nothing here comes from an observed error of a kernel under test: every constant is the precision of the number format,
a count of roundings, or the derivative of the function a bound is propagated through, with its derivation next to it.
``ratio(got, want, bound)`` is the comparator: the largest ``|got - want| / bound``; a test asserts it is <= 1 and
prints it, so that the headroom can be read from a log (DESIGN.md lists the first hardware run).
"""
import numpy as np

U = 2.0 ** -24          # unit roundoff of IEEE binary32, round to nearest

# Factor on the dot-product bound.  The textbook forward bound assumes every product and every addition is rounded to
# nearest.  Whether v_mfma_f32_32x32x2_f32 on gfx950 rounds its internal additions to nearest or truncates them has NOT
# been measured by this project; a truncating adder has unit roundoff 2u instead of u, and c = 2 allows for exactly that.
C_MFMA = 2.0


def dot_bound(absprod, K, bias=None):
    """|fl(sum_k a_k w_k + bias) - exact| <= c * (K + 2) * u * (|a| . |w| + |bias|), for ANY summation order.

    Higham, Accuracy and Stability of Numerical Algorithms, (3.5): a K-term dot product has error gamma_K |a|.|w| whatever
    the order (one rounding per product, at most K - 1 per partial sum chain).  + 1 for the bias addition, + 1 for one
    rounding of an operand prepared in fp64 and stored as fp32 (folded batch norm weights, the windowed DFT basis).
    ``absprod`` is |A| . |W| computed in fp64 by the reference; K is the FULL reduction length."""
    s = np.asarray(absprod, dtype=np.float64)
    if bias is not None:
        s = s + np.abs(np.asarray(bias, dtype=np.float64))
    return C_MFMA * (K + 2) * U * s


def softmax_rel_bound(delta, Tk, spread):
    """Relative error of softmax weights w_j = e^(l_j - m) / sum_i e^(l_i - m) whose logits carry an absolute error <= delta.

    Numerator: e^(+-delta); denominator: a positive sum of terms each within e^(+-delta): together e^(2 delta) - 1 (the
    shift m cancels exactly between the two).  Roundings: the subtraction l_j - m (absolute u * |l_j - m| <= u * spread,
    which exp turns into a relative error), expf (2 ulp = 4u), the sum of Tk positive terms in any order ((Tk - 1) u), the
    reciprocal (2u: not assumed correctly rounded) and the final product (u): (spread + Tk + 8) u, doubled because the
    exp and sum roundings act on numerator and denominator alike."""
    return np.expm1(2.0 * np.asarray(delta, dtype=np.float64)) + 2.0 * (spread + Tk + 8) * U


def context_bound(w, absv_dot, rel_w, Tk):
    """out = sum_j w_j v_j with weights of relative error rel_w: |d out| <= rel_w * (w . |v|) + dot_bound(w . |v|, Tk)."""
    return rel_w * absv_dot + dot_bound(absv_dot, Tk)


def magnitude_bound(re, im, b_re, b_im):
    """|sqrt(re'^2 + im'^2) - sqrt(re^2 + im^2)| <= hypot(b_re, b_im) (reverse triangle inequality of the 2-norm; holds at
    magnitude 0 too, where a first-order bound does not), plus 3u relative: two roundings of re*re + im*im halved by the
    square root (u), and the rounding of sqrtf with one spare ulp (2u)."""
    mag = np.hypot(re, im)
    h = np.hypot(b_re, b_im)
    return h + 3.0 * U * (mag + h)


def power_bound(re, im, b_re, b_im):
    """|(re + e)^2 - re^2| <= 2 |re| e + e^2, the same for im, plus the two roundings of re*re + im*im (3u with a spare)."""
    p = re * re + im * im
    d = 2.0 * np.abs(re) * b_re + b_re ** 2 + 2.0 * np.abs(im) * b_im + b_im ** 2
    return d + 3.0 * U * (p + d)


def mel_bound(basis_abs, spec, b_spec, n_bin):
    """mel = basis . spec (basis_abs (n_mels, n_bin), spec and b_spec (frames, n_bin)): the input error passes through the
    non-negative filters unchanged, basis . b_spec, and the product itself adds dot_bound(basis . |spec|, n_bin)."""
    return b_spec @ basis_abs.T + dot_bound(np.abs(spec) @ basis_abs.T, n_bin)


def log_bound(mel, b_mel, floor, ln_base):
    """log_b(max(mel, floor)).  Returns (bound, usable): d log_b(x) = dx / (x ln b), integrated over [mel - b, mel]:
    -log1p(-b / mel) / ln b; plus 4u * max(|log_b mel|, 1) for logf / log10f (2 ulp) and the float32 rounding of the floor
    constant's neighbourhood.  ``usable`` is False where mel - b_mel <= floor with b_mel > 0: there the clip may or may not
    have acted on the fp32 value and only those entries may be left out (a test asserts they are < 1 % of a case).
    Entries whose reference is exactly 0 with bound 0 (silence, an empty filter) are usable: the clip certainly acts, the
    kernel must return log_b(floor) up to the rounding of logf / log10f (tests compare the log10 of silence exactly)."""
    mel = np.asarray(mel, dtype=np.float64)
    b = np.asarray(b_mel, dtype=np.float64)
    exact_floor = (mel == 0.0) & (b == 0.0)
    usable = (mel - b > floor) | exact_floor
    safe = np.where(usable & ~exact_floor, mel, floor)
    rel = np.where(usable & ~exact_floor, b / safe, 0.0)
    bound = -np.log1p(-rel) / ln_base + 4.0 * U * np.maximum(np.abs(np.log(safe) / ln_base), 1.0)
    return bound, usable


def sinusoid_bound(p):
    """sin / cos of p = (start + pos) * omega / 10000^(channel / size) evaluated in fp32: |p| * 16u + 4u.

    Relative error of the fp32 argument: the product with omega (u), the quotient channel / size (u, amplified by
    ln 10000 * channel / size <= 9.2 in the exponent), powf (2u) and the division (u): 13.2u, rounded up to 16u; sin and cos
    have derivative <= 1, so the argument's absolute error |p| * 16u carries over.  4u: a few ulp of sinf / cosf near 1.
    The reference's own fp32 evaluation of the same formula is in this error class, which is why it is the bar."""
    return np.abs(np.asarray(p, dtype=np.float64)) * 16.0 * U + 4.0 * U


def ratio(got, want, bound, where=None):
    """max |got - want| / bound over the entries selected by ``where``; an entry with bound 0 must match exactly (else inf).
    NaN or inf in ``got`` gives inf."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    assert got.shape == want.shape, f"shape {got.shape} vs {want.shape}"
    if where is not None:
        got, want, bound = got[where], want[where], bound[where]
    if got.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


# ---- mutants: what a subtly wrong GEMM kernel would produce.  A comparator that accepts one of them is too loose.
def mutants(A, W, y):
    """A (M, K), W (K, N), y = A @ W (+ bias) in fp64 -> {name: wrong y}:
       product: the largest-magnitude product of ONE output element is dropped (a lane that skips one k);
       slab:    the middle K slab of 16 is skipped for the first 128-column tile (a slab loop that ends early);
       row:     the last row of the first 128-row tile (the last one with a non-zero result) is left at zero (a tail row
                that is never stored)."""
    A = np.asarray(A, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    M, K = A.shape
    N = W.shape[1]
    out = {}
    r, c = min(M, 128) // 2, min(N, 128) // 2
    prods = A[r] * W[:, c]
    while not prods.any() and c + 1 < N:       # a column of zeros (the imaginary part of DFT bin 0) has nothing to drop
        c += 1
        prods = A[r] * W[:, c]
    m = y.copy()
    m[r, c] -= prods[np.argmax(np.abs(prods))]
    out["product"] = m
    k0 = (K // 16 // 2) * 16
    k1 = min(k0 + 16, K)
    m = y.copy()
    m[:, :128] -= A[:, k0:k1] @ W[k0:k1, :128]
    out["slab"] = m
    m = y.copy()
    last = min(M, 128) - 1
    while last > 0 and not m[last].any():      # a row of pure padding is zero either way: take the last one that is not
        last -= 1
    m[last] = 0.0
    out["row"] = m
    return out
