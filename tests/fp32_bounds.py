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


# ------------------------------------------------------------------------------------------------ split-fp16 GEMM
# Format constants of csrc/pk_split.h: a block maximum is brought to [2^BLK_TOP, 2^(BLK_TOP + 1)); fp32 exponent fields
# below EXP_MIN / above EXP_MAX are clamped (blocks below 2^-40 are scaled as if they were 2^-40).
BLK_TOP, EXP_MIN, EXP_MAX = 13, 87, 200
U16 = 2.0 ** -11        # unit roundoff of IEEE binary16 (11-bit significand), round to nearest
SUB16 = 2.0 ** -25      # half the spacing 2^-24 of binary16 subnormals: absolute rounding error below 2^-14


def act_scale(amax):
    """2^kx the kernel multiplies an activation block with, from the block maximum it is GIVEN (blk_scale_exp: the fp32
    exponent field e of the maximum, clamped to [EXP_MIN, EXP_MAX], kx = BLK_TOP + 127 - e).  Exact, like the kernel."""
    a = np.asarray(amax, dtype=np.float32)
    e = (a.view(np.uint32) >> np.uint32(23)).astype(np.int64) & 0xFF
    return np.ldexp(1.0, BLK_TOP + 127 - np.clip(e, EXP_MIN, EXP_MAX))


def weight_scale(wmax):
    """2^kw of a 128-column weight block (pk_weight_scale_exp): wmax * 2^kw in [2^13, 2^14), |kw| <= 40, 1 for a zero block."""
    w = np.asarray(wmax, dtype=np.float64)
    _, e = np.frexp(w)
    return np.where(w == 0, 1.0, np.ldexp(1.0, np.clip(14 - e, -40, 40)))


def split_dot_bound(absprod, K, sum_abs_a, sum_abs_w, sa, sw, bias=None):
    """Error of sum_k a_k w_k evaluated as a_hi w_hi + a_lo w_hi + a_hi w_lo on fp16 parts of the SCALED operands
    x = sa * a, v = sw * w (sa (M, 1) = act_scale of the row's block, sw (1, N) = weight_scale of the column's block),
    fp32 accumulation, exact unscaling by 1 / (sa * sw).

    Parts: hi = fp16(x) has |x - hi| <= U16 |x| (or <= SUB16 where hi is subnormal); x - hi is exact in fp32 (a multiple
    of ulp32(x) below ulp16(x)); lo = fp16(x - hi) has error <= U16 |x - hi| <= U16^2 |x| = 2^-22 |x| where lo is normal and
    <= SUB16 where it is subnormal.  So e_x = |x - hi - lo| <= 2^-22 |x| + 2^-25, and the same for v.
    Products: hi*hi + lo*hi + hi*lo = (x - e_x)(v - e_v) - lo_x lo_v, i.e. per term an error
        e_x |v| + |x| e_v + e_x e_v + |lo_x lo_v|,   |lo_x| <= U16 (1 + U16) |x| + SUB16  (same for v)
    Summed over k in scaled units, with P = sum |x||v|, SX = sum |x|, SV = sum |v|:
        rep = (3 * 2^-22 (1 + 2^-9)) P + 2^-25 (1 + 2^-9) (SX + SV) + K 2^-49
    (2^-22 P twice for e_x |v| and |x| e_v, once for lo*lo; the factor (1 + 2^-9) and K 2^-49 absorb every second-order
    product of the above: 2^-44 P, 2^-36 (SX + SV) from lo*lo's and e_x e_v's cross terms, 2^-50 K twice).
    Each fp16 x fp16 product has 22 significant bits: exact in fp32.  Accumulation: 3K terms + bias in any order,
    gamma_(3K+2) under the C_MFMA allowance, on sum |parts' products| <= (|hi_x| + |lo_x|)(|hi_v| + |lo_v|) summed,
    |hi| + |lo| <= (1 + 2^-10 + 2^-21)|x| + 2^-24: <= (1 + 2^-9) P + 2^-23 (SX + SV) + K 2^-48.
    Unscaled: P / (sa sw) = |a|.|w| = absprod, SX / (sa sw) = sum|a| / sw, SV / (sa sw) = sum|w| / sa -- the floor terms
    scale with (block maximum of the row) * sum|w| and (block maximum of the column) * sum|a|, as 1 / sa <= amax 2^-13."""
    P = np.asarray(absprod, dtype=np.float64)
    sa = np.asarray(sa, dtype=np.float64)
    sw = np.asarray(sw, dtype=np.float64)
    floor_sum = np.asarray(sum_abs_a, np.float64) / sw + np.asarray(sum_abs_w, np.float64) / sa
    unit = 1.0 / (sa * sw)
    g = 1.0 + 2.0 ** -9
    rep = 3.0 * 2.0 ** -22 * g * P + SUB16 * g * floor_sum + K * 2.0 ** -49 * unit
    mag = g * P + 2.0 ** -23 * floor_sum + K * 2.0 ** -48 * unit
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, dtype=np.float64))
    return rep + C_MFMA * (3 * K + 2) * U * mag


# __expf(x) = exp2(x * log2(e)).  ROCm's documentation on this machine states no error for it; this is the derivation
# from the instruction: v_exp_f32 is 1 ulp (2u relative); its argument t = x * log2(e) carries the rounding of the
# constant and of the product (2u relative, |dt| <= 2u |t|), which exp2 turns into the relative error ln 2 * |dt| =
# 2u |x|.  Results that underflow are flushed: an absolute 2^-126, nothing next to the u-sized terms around it.
def fast_exp_rel(x):
    return 2.0 * U * (np.abs(np.asarray(x, dtype=np.float64)) + 1.0)


TANH_CLAMP = 10.0


def gate_bound(ca, cb, b_ca, b_cb):
    """z = tanh(ca) * sigmoid(cb) from pre-activations with absolute errors b_ca, b_cb, computed as
    ea = __expf(-2 clamp(ca, +-10)), eb = __expf(-cb), z = (1 - ea) / ((1 + ea)(1 + eb)).
    T = (1 - ea) / (1 + ea): dT/dca <= 1; dT/dea * ea = 2 ea / (1 + ea)^2 <= 1/2, so ea's relative error d_a costs d_a / 2;
    the clamp changes tanh by at most 1 - tanh(10) where |ca| can reach 10.  S = 1 / (1 + eb): dS/dcb <= 1/4,
    dS/deb * eb = S (1 - S) <= 1/4.  Roundings of 1 - ea, 1 + ea, 1 + eb, the product (u each) and the division (2u: not
    assumed correctly rounded): 6u relative to z."""
    ca, cb = np.asarray(ca, np.float64), np.asarray(cb, np.float64)
    T, S = np.tanh(ca), 1.0 / (1.0 + np.exp(-cb))
    clamp = np.where(np.abs(ca) + b_ca >= TANH_CLAMP, 1.0 - np.tanh(TANH_CLAMP), 0.0)
    bT = b_ca + 0.5 * fast_exp_rel(2.0 * np.minimum(np.abs(ca) + b_ca, TANH_CLAMP)) + clamp
    bS = 0.25 * b_cb + 0.25 * fast_exp_rel(np.abs(cb) + b_cb)
    return np.abs(S) * bT + np.abs(T) * bS + bT * bS + 6.0 * U * np.abs(T * S)


def epilogue_step(v, b, rounding=1):
    """after an operation whose exact result is v from operands with propagated error b: + `rounding` roundings of it"""
    return b + rounding * U * (np.abs(v) + b)


# tanhf / expf of the device library: the documentation at hand states no error for them; the allowance is the 2 ulp = 4u
# relative this file already grants expf (softmax_rel_bound) and logf (log_bound); |tanh| <= 1 makes it an absolute 4u.
LIBM_REL = 4.0 * U


def tanh_bound(x, b):
    """|d tanh| <= 1 * b (derivative <= 1) + 4u"""
    return b + LIBM_REL


def sigmoid_bound(x, b):
    """1 / (1 + expf(-x)): derivative <= 1/4; expf's relative error e acts as S (1 - S) e <= e / 4; 1 + . and 1 / . : 3u"""
    return 0.25 * b + 0.25 * LIBM_REL + 3.0 * U


def layernorm_bound(x, g, beta, eps):
    """xn = (x - mean) * rstd * g + beta over the last axis (K) in fp32 -> (xn fp64, bound).
    mean: K additions in any order and the product with the rounded 1/K: (K + 2) u mean|x|.  d = x - mean: b_d = b_mean +
    u |d|.  var = mean(d^2): each square moves by 2 |d| b_d + b_d^2 (+ u d^2), the sum and 1/K add (K + 2) u var.
    rstd = 1 / sqrt(var + eps): |d rstd / d var| = rstd^3 / 2, taken at the smallest variance the error allows; the
    addition of eps, sqrtf and the division: 4u relative (sqrtf and the division are not assumed correctly rounded).
    The three products and the addition of beta: 3u on the product, u on the sum."""
    x = np.asarray(x, np.float64)
    K = x.shape[-1]
    mean = x.mean(-1, keepdims=True)
    b_mean = (K + 2) * U * np.abs(x).mean(-1, keepdims=True)
    d = x - mean
    b_d = b_mean + U * np.abs(d)
    var = (d * d).mean(-1, keepdims=True)
    b_var = (2 * np.abs(d) * b_d + b_d ** 2 + U * d * d).mean(-1, keepdims=True) + (K + 2) * U * var
    rstd = 1.0 / np.sqrt(var + eps)
    rs_hi = 1.0 / np.sqrt(np.maximum(var - b_var, 0.0) + eps)
    b_rs = 0.5 * rs_hi ** 3 * b_var + 4.0 * U * rs_hi
    g, beta = np.asarray(g, np.float64), np.asarray(beta, np.float64)
    core = d * rstd * g
    b_core = np.abs(g) * (b_d * rstd + np.abs(d) * b_rs + b_d * b_rs) + 3.0 * U * np.abs(core)
    xn = core + beta
    return xn, b_core + U * (np.abs(xn) + b_core)


def lstm_bound(gi, gf, gg, go, b_pre, c, b_c):
    """One LSTMCell step from gate pre-activations (each with absolute error b_pre) and the cell state c (error b_c):
    c' = sigmoid(f) c + sigmoid(i) tanh(g), h = sigmoid(o) tanh(c') -> (c', h, b_c', b_h).
    Product rule with the derivative bounds of sigmoid_bound / tanh_bound; two products and a sum for c' (u each on its
    operands: 3u (|f c| + |i g|)), tanhf(c') and a product for h."""
    si, sf, so = (1.0 / (1.0 + np.exp(-np.asarray(v, np.float64))) for v in (gi, gf, go))
    tg = np.tanh(np.asarray(gg, np.float64))
    b_s, b_t = sigmoid_bound(None, b_pre), tanh_bound(None, b_pre)
    c = np.asarray(c, np.float64)
    cn = sf * c + si * tg
    b_cn = (np.abs(c) * b_s + sf * b_c + b_s * b_c) + (np.abs(tg) * b_s + si * b_t + b_s * b_t)
    b_cn = b_cn + 3.0 * U * (np.abs(sf * c) + np.abs(si * tg) + b_cn)
    tc = np.tanh(cn)
    b_tc = tanh_bound(None, b_cn)
    h = so * tc
    b_h = np.abs(tc) * b_s + so * b_tc + b_s * b_tc
    return cn, h, b_cn, b_h + U * (np.abs(h) + b_h)


def split_emulation(A, W, sa, sw):
    """numpy emulation of the split product (for the CPU proof): scale, np.float16 hi / lo, three float32 products
    accumulated in float32, exact unscale.  A (M, K) float32, W (K, N) float32, sa (M, 1), sw (1, N)."""
    x = (A.astype(np.float64) * sa).astype(np.float32)
    v = (W.astype(np.float64) * sw).astype(np.float32)
    xh = x.astype(np.float16).astype(np.float32)
    xl = (x - xh).astype(np.float16).astype(np.float32)
    vh = v.astype(np.float16).astype(np.float32)
    vl = (v - vh).astype(np.float16).astype(np.float32)
    acc = xh @ vh + xl @ vh + xh @ vl
    assert acc.dtype == np.float32
    return (acc.astype(np.float64) / (sa * sw)).astype(np.float32)


def _fp16_hi(x):
    """x rounded to the fp16 grid of its own binade (a power-of-two block scale does not change it)"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.round(m * 2048.0) / 2048.0, e)


def split_mutants(A, W, y, sa_own=None, sw=None, sa=None, slab=None):
    """Wrong results specific to the split kernel, {name: wrong y} (y = A @ W in fp64, same shapes as mutants()):
       lohi:     the lo*hi term of one 32-wide K slab (default: the middle one) is missing for the first 64-row tile
                 (the activations' low parts of that slab dropped);
       hilo:     the hi*lo term of that slab is missing for the first 128-column tile (the weights' low parts dropped);
       ownscale: the row scale comes from the row itself (sa_own) instead of the rows its taps read (sa): where the
                 neighbour is larger, scaled values overflow fp16 -- emulated, returned only when sa_own is given."""
    A32, W32 = np.asarray(A, np.float32).astype(np.float64), np.asarray(W, np.float32).astype(np.float64)
    K = A32.shape[1]
    out = {}
    k0 = (K // 32 // 2 if slab is None else slab) * 32
    ks = slice(k0, k0 + 32)
    wrong = y.copy()
    wrong[:64] -= (A32[:64, ks] - _fp16_hi(A32[:64, ks])) @ _fp16_hi(W32[ks])
    out["lohi"] = wrong
    wrong = y.copy()
    wrong[:, :128] -= _fp16_hi(A32[:, ks]) @ (W32[ks, :128] - _fp16_hi(W32[ks, :128]))
    out["hilo"] = wrong
    if sa_own is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            out["ownscale"] = split_emulation(np.asarray(A, np.float32), np.asarray(W, np.float32), sa_own, sw).astype(np.float64)
    return out


def gemm_epilogue_mutants(want, res=None, gap_rows=None, c2_old=None, c2_new=None):
    """(c) a gap row keeps its residual; (d) C2 overwritten where acc2 asks for += ."""
    out = {}
    if res is not None and gap_rows is not None and len(gap_rows):
        m = want.copy()
        m[gap_rows] = np.asarray(res, np.float64)[gap_rows]
        out["gapres"] = m
    if c2_old is not None:
        out["c2over"] = np.asarray(c2_new, np.float64) - np.asarray(c2_old, np.float64)
    return out


def lstm_swap_mutant(W, H):
    """(e) the i and f gate columns of every unit swapped: W (K, 4H) in [i | f | g | o] order -> wrong W"""
    W = np.asarray(W).copy()
    W[:, :H], W[:, H:2 * H] = np.asarray(W)[:, H:2 * H].copy(), np.asarray(W)[:, :H].copy()
    return W
