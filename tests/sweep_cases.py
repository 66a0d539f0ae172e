"""Cases, seeded inputs and fp64 references of the primitive / STFT sweeps, shared by tests/test_fp32_bounds_cpu.py (which
checks on the host that the derived bounds accept an fp32 evaluation and reject wrong results for EVERY case) and by
tests/test_ops_sweep_gpu.py / tests/test_audio_sweep_gpu.py (which run the same cases on the kernels).

The references restate the formulas of parakeet/modules (attention.py:22-58, conv.py:22-260, expansion.py:19-37,
positional_encoding.py:20-39, audio.py:74-229) and parakeet/data/get_feats.py:20-88 in numpy fp64.
GEMM-type inputs have a non-zero mean, so that results are comparable with the abs-product |A| . |W| their bound scales
with; with zero-mean data the bound would dwarf the result and hide a wrong kernel.
"""
import itertools
import math
import zlib
from collections import namedtuple

import numpy as np

import fp32_bounds as fb


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ attention
ATT_TK, ATT_D, ATT_DV = (1, 63, 64, 65, 200, 1000), (8, 64, 80, 192), (1, 64, 65, 160)
ATT_ROWS = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (1, 5), 130: (2, 65)}        # B * Tq -> (B, Tq)
ATT_MASKS = ("none", "b1k", "bqk", "qk")     # none, (B,1,Tk), (B,Tq,Tk) different per batch, shared causal (Tq,Tk)
AttCase = namedtuple("AttCase", "Tk d dv rows mask")


def _attention_cases():
    """Every (Tk, d) and (Tk, dv) pair once (24 shape triples), then mask mode and row count assigned greedily so that
    every value of every axis meets every mask mode; triples are reused (smallest first) until that holds."""
    triples = [(tk, ATT_D[j], ATT_DV[(i + j) % 4]) for i, tk in enumerate(ATT_TK) for j in range(4)]
    need = set()
    for m in ATT_MASKS:
        need |= {("Tk", v, m) for v in ATT_TK} | {("d", v, m) for v in ATT_D} | {("dv", v, m) for v in ATT_DV}
        need |= {("rows", v, m) for v in ATT_ROWS}

    def covers(tk, d, dv, rows, m):
        return {("Tk", tk, m), ("d", d, m), ("dv", dv, m), ("rows", rows, m)}

    cases = []
    options = list(itertools.product(ATT_ROWS, ATT_MASKS))

    def gain(t, rm):        # new combinations first, then the row counts and mask modes used least so far
        return (len(covers(*t, *rm) & need), -sum(c.rows == rm[0] for c in cases), -sum(c.mask == rm[1] for c in cases))

    # a second pass over the shapes with the other (d, dv) pairing spreads rows and masks further (about 50 cases)
    for t in triples + [(tk, ATT_D[j], ATT_DV[(i + j + 2) % 4]) for i, tk in enumerate(ATT_TK) for j in range(4)]:
        best = max(options, key=lambda rm: gain(t, rm))
        need -= covers(*t, *best)
        cases.append(AttCase(*t, *best))
    small = sorted(triples, key=lambda t: t[0] * (t[1] + t[2]))
    while need:
        t, best = max(((t, rm) for t in small for rm in options), key=lambda x: gain(*x)[0])
        need -= covers(*t, *best)
        cases.append(AttCase(*t, *best))
    return cases


ATT_CASES = _attention_cases()
ATT_LDS_EDGE = AttCase(4000, 96, 8, 4, "b1k")       # d + Tk == 4096: the largest problem the 64 KB of LDS hold


def att_id(c):
    return f"Tk{c.Tk}-d{c.d}-dv{c.dv}-rows{c.rows}-{c.mask}"


def attention_inputs(c):
    B, Tq = ATT_ROWS[c.rows]
    r = rng_for("att", *c)
    q = f32(r.normal(0.3, 1.0, (B, Tq, c.d)))
    k = f32(r.normal(0.3, 1.0, (B, c.Tk, c.d)))
    v = f32(r.normal(0.5, 1.0, (B, c.Tk, c.dv)))
    mask = None
    if c.mask == "b1k":
        mask = np.ones((B, 1, c.Tk), np.float32)
        for b in range(B):
            mask[b, 0, max(1, (c.Tk * (b + 3)) // (B + 3)):] = 0          # a different padded length per batch
    elif c.mask == "bqk":
        mask = f32(r.uniform(size=(B, Tq, c.Tk)) < 0.7)                    # different per batch and per query
        mask[..., 0] = 1
        mask[B - 1, Tq - 1, :] = 0                                         # ONE fully masked row
    elif c.mask == "qk":
        mask = np.tril(np.ones((Tq, c.Tk), np.float32), k=max(0, c.Tk - Tq))   # causal, every row keeps >= 1 key
    return q, k, v, mask


def attention_reference(q, k, v, mask):
    """-> dict(out, w, b_out, b_w, stages) in fp64.  A fully masked row has exactly uniform weights 1 / Tk under the fp32
    semantics of the reference (attention.py:52-54 adds (1 - mask) * -1e9 in float32: |s| << ulp(1e9) = 64, so s - 1e9
    rounds to -1e9 for every key and the softmax sees equal logits); elsewhere masked keys have weight exactly 0
    (e^(-1e9) underflows)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    B, Tq, d = q.shape
    Tk = k.shape[1]
    scale = 1.0 / math.sqrt(d)
    logit = np.einsum("bqc,bkc->bqk", q, k) * scale
    absdot = np.einsum("bqc,bkc->bqk", np.abs(q), np.abs(k)) * scale
    # the dot product, then the rounded factor 1/sqrtf(d) (2u relative with its own rounding) and the product (u)
    delta = fb.dot_bound(absdot, d) + 3.0 * fb.U * np.abs(logit)
    keep = np.ones((B, Tq, Tk), bool) if mask is None else np.broadcast_to(np.asarray(mask) != 0, (B, Tq, Tk))
    dead = ~keep.any(-1)                                                   # fully masked rows
    lm = np.where(keep, logit, -np.inf)
    lm[dead] = 0.0
    mx = lm.max(-1, keepdims=True)
    e = np.exp(lm - mx)
    w = e / e.sum(-1, keepdims=True)
    live = keep | dead[..., None]
    spread = np.where(live, mx - lm, 0.0).max(-1, keepdims=True)
    dmax = np.where(keep, delta, 0.0).max(-1, keepdims=True)
    rel = fb.softmax_rel_bound(dmax, Tk, spread)
    rel = np.where(dead[..., None], 2.0 * (Tk + 8) * fb.U, rel)            # equal logits: only the sum / divide roundings
    out = np.einsum("bqk,bkc->bqc", w, v)
    absv = np.einsum("bqk,bkc->bqc", w, np.abs(v))
    return dict(out=out, w=w, b_w=w * rel, b_out=fb.context_bound(w, absv, rel, Tk), dead=dead,
                stages=[("logits", q[0], k[0].T * scale, logit[0], absdot[0], d),
                        ("context", w[0], v[0], out[0], absv[0], Tk)])


# ------------------------------------------------------------------------------------------------ Conv1dBatchNorm / Linear
CONV_CIN, CONV_COUT, CONV_K = (16, 80, 256), (1, 127, 128, 129, 300), (1, 2, 3, 5, 12)
ConvCase = namedtuple("ConvCase", "Cin Cout k pad T B bias bn layout")


def conv_pads(k):
    """0, 1, 'same' and 'full' padding, then the range the row timeline could not hold before its gap was sized from
    the padding: pad = k (one output row more than T + k) and pad = k + 2 (taps that read more than k rows back)."""
    return sorted({0, 1, (k - 1) // 2, k - 1, k, k + 2})


def conv_ts(k):
    return sorted({1, k, 37, 128 - k, 500})


def _conv_cases():
    cases = []
    for ki, k in enumerate(CONV_K):
        combos = [(p, t) for p in conv_pads(k) for t in conv_ts(k) if t + 2 * p - k + 1 >= 1]
        for n, (p, t) in enumerate(combos):
            i = len(cases)
            big = t == 500
            cases.append(ConvCase(Cin=CONV_CIN[(n + ki) % 3] if not (big and k == 12) else 16,
                                  Cout=CONV_COUT[(n + ki) % 5], k=k, pad=p, T=t,
                                  B=3 if (p >= k or i % 2) else 1, bias=i % 3 != 0, bn=i % 4 < 2,
                                  layout="NCL" if i % 5 < 2 else "NLC"))
    return cases


CONV_CASES = _conv_cases()


def conv_id(c):
    return (f"Cin{c.Cin}-Cout{c.Cout}-k{c.k}-pad{c.pad}-T{c.T}-B{c.B}-{'bias' if c.bias else 'nobias'}-"
            f"{'bn' if c.bn else 'nobn'}-{c.layout}")


def conv_inputs(c):
    r = rng_for("conv", *c)
    K = c.Cin * c.k
    st = {"conv.weight": f32(r.normal(0.3, 1.0, (c.Cout, c.Cin, c.k)) / math.sqrt(K))}
    if c.bias:
        st["conv.bias"] = f32(r.normal(0.2, 1.0, c.Cout))
    if c.bn:
        st.update({"bn.weight": f32(r.uniform(0.5, 1.5, c.Cout)), "bn.bias": f32(r.normal(size=c.Cout)),
                   "bn._mean": f32(r.normal(size=c.Cout)), "bn._variance": f32(r.uniform(0.5, 1.5, c.Cout))})
    x = f32(r.normal(0.5, 1.0, (c.B, c.T, c.Cin)))                        # NLC
    return x, st


def conv_reference(x_nlc, st, k, pad, eps=1e-5):
    """-> (want (B, Tout, Cout), bound, A (B*Tout, k*Cin), W (k*Cin, Cout), shift): the convolution as the im2col product
    it is, with eval-mode batch norm folded the way the engine folds it (in fp64), so that |A| . |W'| + |shift| is the
    abs-product of what the kernel sums."""
    x = np.asarray(x_nlc, np.float64)
    B, T, Cin = x.shape
    w = np.asarray(st["conv.weight"], np.float64)
    Cout = w.shape[0]
    tout = T + 2 * pad - k + 1
    xp = np.pad(x, ((0, 0), (pad, pad), (0, 0)))
    A = np.stack([xp[:, t:t + tout] for t in range(k)], axis=2).reshape(B * tout, k * Cin)     # [tap][ci]
    W = w.transpose(2, 1, 0).reshape(k * Cin, Cout)
    s = np.ones(Cout)
    sh = np.asarray(st["conv.bias"], np.float64) if "conv.bias" in st else np.zeros(Cout)
    if "bn.weight" in st:
        s = np.asarray(st["bn.weight"], np.float64) / np.sqrt(np.asarray(st["bn._variance"], np.float64) + np.float32(eps))
        sh = (sh - np.asarray(st["bn._mean"], np.float64)) * s + np.asarray(st["bn.bias"], np.float64)
    W = W * s
    want = A @ W + sh
    bound = fb.dot_bound(np.abs(A) @ np.abs(W), k * Cin, sh)
    return want.reshape(B, tout, Cout), bound.reshape(B, tout, Cout), A, W, sh


# ------------------------------------------------------------------------------------------------ matmul
MM_M, MM_K, MM_N = (1, 127, 128, 129, 1000), (1, 15, 16, 17, 513, 1025), (1, 80, 128, 129, 402)
MmCase = namedtuple("MmCase", "M K N bias")
# every (K, N) pair once; for a fixed N the six K values walk through all five M values, so every (M, N) pair occurs too
MM_CASES = [MmCase(MM_M[(ki + ni) % 5], K, N, bias) for ni, N in enumerate(MM_N) for ki, K in enumerate(MM_K)
            for bias in (False, True)]


def mm_id(c):
    return f"M{c.M}-K{c.K}-N{c.N}-{'bias' if c.bias else 'nobias'}"


def matmul_inputs(c):
    r = rng_for("mm", c.M, c.K, c.N)
    return (f32(r.normal(0.5, 1.0, (c.M, c.K))), f32(r.normal(0.3, 1.0, (c.K, c.N)) / math.sqrt(c.K)),
            f32(r.normal(0.2, 1.0, c.N)) if c.bias else None)


def matmul_reference(x, w, bias):
    A, W = np.asarray(x, np.float64), np.asarray(w, np.float64)
    b = np.zeros(W.shape[1]) if bias is None else np.asarray(bias, np.float64)
    return A @ W + b, fb.dot_bound(np.abs(A) @ np.abs(W), A.shape[1], b)


# ------------------------------------------------------------------------------------------------ Conv1dCell
CellCase = namedtuple("CellCase", "Cin k dil B Cout bias")
CELL_CASES = [CellCase(64, 3, 1, 1, 1, True), CellCase(80, 2, 7, 5, 1, True), CellCase(5, 9, 3, 2, 4, False),
              CellCase(128, 1, 1, 3, 43, True), CellCase(64, 3, 1, 1, 5, False), CellCase(80, 2, 7, 3, 43, False),
              CellCase(5, 9, 3, 1, 1, True), CellCase(128, 1, 1, 2, 4, False)]


def cell_id(c):
    return f"Cin{c.Cin}-k{c.k}-dil{c.dil}-B{c.B}xCout{c.Cout}-{'bias' if c.bias else 'nobias'}"


def cell_inputs(c, tag=0):
    r = rng_for("cell", tag, *c)
    rf = 1 + (c.k - 1) * c.dil
    st = {"weight": f32(r.normal(0.3, 1.0, (c.Cout, c.Cin, c.k)) / math.sqrt(c.Cin * c.k))}
    if c.bias:
        st["bias"] = f32(r.normal(0.2, 1.0, c.Cout))
    return f32(r.normal(0.5, 1.0, (c.B, c.Cin, 2 * rf))), st


def cell_reference(x_ncl, st, k, dil):
    """Causal dilated convolution of the whole sequence (left padding receptive_field - 1): -> want, bound (B, Cout, T),
    and the im2col operands A (B*T, Cin*k), W (Cin*k, Cout)."""
    x = np.asarray(x_ncl, np.float64)
    B, Cin, T = x.shape
    w = np.asarray(st["weight"], np.float64)
    Cout = w.shape[0]
    xp = np.pad(x, ((0, 0), (0, 0), ((k - 1) * dil, 0)))
    A = np.stack([xp[:, :, j * dil:j * dil + T] for j in range(k)], axis=2)       # (B, Cin, k, T)
    A = A.transpose(0, 3, 1, 2).reshape(B * T, Cin * k)
    W = w.reshape(Cout, Cin * k).T
    b = np.asarray(st["bias"], np.float64) if "bias" in st else np.zeros(Cout)
    want = (A @ W + b).reshape(B, T, Cout).transpose(0, 2, 1)
    bound = fb.dot_bound(np.abs(A) @ np.abs(W), Cin * k, b).reshape(B, T, Cout).transpose(0, 2, 1)
    return want, bound, A, W, b


# ------------------------------------------------------------------------------------------------ STFT / mel
MelCfg = namedtuple("MelCfg", "sr n_fft hop win center n_mels total_frames")
# total_frames: the batch is sized so that its frames add up to exactly this (128: the last frame is the last row of a
# GEMM row tile; 129: one row into the next tile); None: the long utterance alone has 140 frames
MEL_CFGS = [MelCfg(22050, 1024, 256, 1024, True, 80, 128), MelCfg(24000, 2048, 300, 1200, True, 80, 129),
            MelCfg(16000, 400, 160, 400, True, 40, None), MelCfg(16000, 48, 12, 48, True, 10, None),
            MelCfg(22050, 512, 128, 400, False, 80, 129), MelCfg(22050, 1024, 256, 1024, False, 80, None)]
MEL_FMIN, MEL_FMAX, MEL_FLOOR = 80, 7600, float(np.float32(1e-10))


def mel_id(c):
    return f"sr{c.sr}-fft{c.n_fft}-hop{c.hop}-win{c.win}-{'center' if c.center else 'nocenter'}"


def num_frames(c, n):
    padded = n + (2 * (c.n_fft // 2) if c.center else 0)
    return 0 if padded < c.n_fft else 1 + (padded - c.n_fft) // c.hop


def mel_batch(c):
    """[shortest legal, all-zero, (center=False: shorter than n_fft -> zero frames), full-scale +-1, long]: the long one
    comes last and crosses the 128-row tile."""
    r = rng_for("mel", *c)
    pad2 = 2 * (c.n_fft // 2) if c.center else 0
    lens = [c.n_fft // 2 + 1 if c.center else c.n_fft, (3 * c.n_fft) // 2 + 7]
    if not c.center:
        lens.append(c.n_fft - 1)
    lens.append(2 * c.n_fft + 3 * c.hop + 1)
    have = sum(num_frames(c, n) for n in lens)
    want_long = 140 if c.total_frames is None else c.total_frames - have
    lens.append((want_long - 1) * c.hop + c.n_fft - pad2 + 5)
    wavs = [f32(np.clip(r.normal(0.0, 0.3, n), -1, 1)) for n in lens]
    wavs[1][:] = 0.0
    wavs[-2] = f32(r.choice([-1.0, 1.0], size=lens[-2]))
    assert c.total_frames is None or sum(num_frames(c, n) for n in lens) == c.total_frames
    return wavs


def window_f32(c):
    import scipy.signal
    w = scipy.signal.get_window("hann", c.win, fftbins=True)
    left = (c.n_fft - c.win) // 2
    return f32(np.pad(w, (left, c.n_fft - c.win - left)))


def mel_reference(c, wav, basis_f32, power=False):
    """One utterance -> dict of fp64 results and bounds (frames-major, like the C ABI), following audio.py:161-215 and
    get_feats.py:75-87: reflect pad, frames . (DFT basis * window), magnitude / power, basis . magnitude, clip, log."""
    x = np.asarray(wav, np.float64)
    N, nb = c.n_fft, 1 + c.n_fft // 2
    if c.center:
        x = np.pad(x, (N // 2, N // 2), mode="reflect")
    F = 0 if len(x) < N else 1 + (len(x) - N) // c.hop
    A = np.stack([x[f * c.hop:f * c.hop + N] for f in range(F)]) if F else np.zeros((0, N))
    n, k = np.arange(N)[:, None], np.arange(nb)[None, :]
    ang = -2.0 * np.pi * ((n * k) % N) / N
    win = window_f32(c).astype(np.float64)[:, None]
    W = np.concatenate([np.cos(ang) * win, np.sin(ang) * win], axis=1)            # (n_fft, re | im)
    reim = A @ W
    absdot = np.abs(A) @ np.abs(W)
    b_reim = fb.dot_bound(absdot, N)
    re, im, b_re, b_im = reim[:, :nb], reim[:, nb:], b_reim[:, :nb], b_reim[:, nb:]
    if power:
        spec, b_spec = re * re + im * im, fb.power_bound(re, im, b_re, b_im)
    else:
        spec, b_spec = np.hypot(re, im), fb.magnitude_bound(re, im, b_re, b_im)
    basis = np.asarray(basis_f32, np.float64)
    mel = spec @ basis.T
    b_mel = fb.mel_bound(np.abs(basis), spec, b_spec, nb)
    clipped = np.maximum(mel, MEL_FLOOR)
    b10, usable = fb.log_bound(mel, b_mel, MEL_FLOOR, math.log(10.0))
    be, _ = fb.log_bound(mel, b_mel, MEL_FLOOR, 1.0)
    return dict(frames=F, reim=reim, b_reim=b_reim, spec=spec, b_spec=b_spec, mel=mel, b_mel=b_mel,
                log10=np.log10(clipped), b_log10=b10, ln=np.log(clipped), b_ln=be, usable=usable,
                stages=[("stft", A, W, reim, absdot, N), ("mel", spec, basis.T, mel, np.abs(spec) @ np.abs(basis.T), nb)])


# ------------------------------------------------------------------------------------------------ sinusoid / expand
SIN_CASES = list(itertools.product((2, 62, 130, 384), (1, 1000), (0, 4095), (1.0, 0.5)))
EXPAND_C = (1, 128, 129, 384)


def sinusoid_reference(num_positions, size, omega, start_pos):
    channel = np.arange(0, size, 2, dtype=np.float64)
    index = np.arange(start_pos, start_pos + num_positions, dtype=np.float64)
    p = (index[:, None] * omega) / (10000.0 ** (channel / size))
    want, arg = np.zeros((num_positions, size)), np.zeros((num_positions, size))
    want[:, 0::2], want[:, 1::2] = np.sin(p), np.cos(p)
    arg[:, 0::2], arg[:, 1::2] = p, p
    return want, fb.sinusoid_bound(arg)


def expand_reference(x, d):
    """expansion.py:19-37: the dense 0/1 matrix the reference builds, applied as a gather (each output row is one input
    row or zero, so the product is exact)."""
    B, T, C = x.shape
    t_dec = int(d.sum(-1).max())
    out = np.zeros((B, t_dec, C), np.float32)
    for b in range(B):
        k = 0
        for t in range(T):
            out[b, k:k + d[b, t]] = x[b, t]
            k += d[b, t]
    return out


# ------------------------------------------------------------------------------------------------ split-fp16 GEMM (pk_op_gemm)
GEMM_M, GEMM_N = (1, 63, 64, 65, 127, 128, 129, 300), (1, 127, 128, 129, 300)
# (Cin, taps, pad) with K = taps * Cin >= 128 (below that the launcher takes the fp32 kernel): K slabs of 32: 5, 6, 10, 15, 25
GEMM_KSHAPES = [(32, 5, 0), (32, 5, 2), (32, 5, 4), (64, 3, 0), (64, 3, 1), (64, 3, 2), (64, 5, 0), (64, 5, 2), (64, 5, 4),
                (160, 1, 0), (160, 3, 0), (160, 3, 1), (160, 3, 2), (160, 5, 0), (160, 5, 2), (160, 5, 4)]
GEMM_RES_POS = (0, 1, 2)       # PK_RES_AFTER_ACT, PK_RES_AFTER_AFFINE, PK_RES_BEFORE_ACT
GemmCase = namedtuple("GemmCase", "M N Cin taps pad res_pos act affine bias res gaps rowmap loud", defaults=(-1,))
# loud: the 32-wide K slab gemm_loud_slab makes loud (-1: the middle one, the slab the standing mutants remove)


def _gemm_cases():
    """Every (M, N) pair once, the K shapes, res_pos and act dealt round so that every value of M, N, Cin, (taps, pad) meets
    every res_pos (test_sweeps_cover_what_they_promise checks it); each case runs at both tile sizes and at tile = 0."""
    cases = []
    for mi, M in enumerate(GEMM_M):
        for ni, N in enumerate(GEMM_N):
            i = len(cases)
            Cin, taps, pad = GEMM_KSHAPES[(3 * mi + 7 * ni + mi * ni) % len(GEMM_KSHAPES)]
            if M == 1:                            # a single row sees only the tap that reads itself: centre it, so that
                pad = (taps - 1) // 2             # the middle K slab (the one the mutants remove) is not padding
            cases.append(GemmCase(M, N, Cin, taps, pad, res_pos=(mi + ni) % 3, act=(mi + 2 * ni) % 3, affine=i % 2 == 0,
                                  bias=i % 3 != 1, res=i % 4 != 3, gaps=i % 2 == 1 or M == 300, rowmap=i % 5 == 0))
    extra = 0
    for ks in GEMM_KSHAPES:                       # K shapes the walk above missed for some res_pos
        for rp in GEMM_RES_POS:
            if not any((c.Cin, c.taps, c.pad) == ks and c.res_pos == rp for c in cases):
                M, N = GEMM_M[1 + extra % 7], GEMM_N[extra % 5]
                extra += 1
                cases.append(GemmCase(M, N, *ks, res_pos=rp, act=extra % 3, affine=True, bias=True, res=True, gaps=True,
                                      rowmap=False))
    return cases


GEMM_CASES = _gemm_cases()
# Small K, where a lost low-part product of ANY slab is above the accumulation term of the bound: 4, 5, 6 and 7 slabs
# (Cin = 32, one slab per tap), every slab loud in turn -- the first, the three of the unrolled ring and both of its tails.
GEMM_TAIL_CASES = [GemmCase((65, 129, 130)[(ns + sl) % 3], (129, 127, 300)[(ns + sl) % 3], 32, ns, ns // 2, res_pos=(ns + sl) % 3,
                            act=0, affine=sl % 2 == 0, bias=True, res=True, gaps=True, rowmap=False, loud=sl)
                   for ns in (4, 5, 6, 7) for sl in range(ns)]


def gemm_id(c):
    return (f"M{c.M}-N{c.N}-Cin{c.Cin}-k{c.taps}-pad{c.pad}-rp{c.res_pos}-act{c.act}-{'aff' if c.affine else 'noaff'}-"
            f"{'bias' if c.bias else 'nobias'}-{'res' if c.res else 'nores'}-{'gaps' if c.gaps else 'nogaps'}-"
            f"{'map' if c.rowmap else 'nomap'}" + (f"-loud{c.loud}" if c.loud >= 0 else ""))


def gemm_gap_rows(M):
    """tile-boundary rows and the last one"""
    return sorted({r for r in (63, 64, 127, 128, M - 1) if 0 <= r < M})


def gemm_problem(c):
    """-> dict of float32 / int32 arrays, the fields of pk_op_gemm_cfg (host and device side alike)."""
    r = rng_for("gemm", *c)
    K = c.taps * c.Cin
    p = dict(M=c.M, N=c.N, Cin=c.Cin, taps=c.taps, pad=c.pad, lda=c.Cin, act=c.act, res_pos=c.res_pos,
             A=f32(r.normal(0.5, 1.0, (c.M, c.Cin))), W=f32(r.normal(0.3, 1.0, (K, c.N)) / math.sqrt(K)))
    p["loud"] = gemm_loud_slab(p["A"], p["W"], c.Cin, c.taps * c.Cin, c.loud)
    if c.bias:
        p["bias"] = f32(r.normal(0.2, 0.5, c.N))
    if c.res:
        p["res"], p["ldr"] = f32(r.normal(0.3, 1.0, (c.M, c.N + 3))), c.N + 3
    if c.affine:
        p["cscale"], p["cshift"] = f32(r.uniform(0.5, 1.5, c.N)), f32(r.normal(0.1, 1.0, c.N))
    if c.gaps:
        rv = np.zeros(c.M, np.int32)
        rv[gemm_gap_rows(c.M)] = -1
        p["rowvalid"] = rv
    if c.rowmap:
        m = np.arange(c.M, dtype=np.int32)[::-1].copy()          # reversed, every third row not stored
        m[::3] = -1
        p["out_rowmap"] = m
    return p


def _half_step_up(v):
    """positive values just under half an fp16 step above an fp16 value: low parts all positive and as large as they get"""
    m, e = np.frexp(np.asarray(v, np.float64))
    return np.ldexp((np.floor(m * 2048.0) + 0.49) / 2048.0, e)


def gemm_loud_slab(A, W, Cin, K, slab=-1, A2=None, Kmain=None):
    """Make one 32-wide K slab of the im2col product loud and one-signed, in place; returns its index.  The worst-case
    accumulation bound grows with K * |A|.|W| while the low-part products of ONE slab do not, so on flat inputs a kernel
    that lost them would pass.  The slab's weights become positive and 2K times the rest (weight rows belong to one tap;
    the activation columns are shared by all taps); the slab's activations and weights both sit just under half an fp16
    step above an fp16 value, so neither operand's low parts cancel.  slab < 0: the middle slab, K // 32 // 2 (the one the
    standing mutants remove).  K counts the rows of the im2col product; rows >= Kmain belong to the A2 block."""
    slab = K // 32 // 2 if slab < 0 else slab
    k0 = slab * 32
    Kmain = K if Kmain is None else Kmain
    X, c0 = (A, k0 % Cin) if k0 < Kmain else (A2, k0 - Kmain)
    X[:, c0:c0 + 32] = _half_step_up(np.abs(X[:, c0:c0 + 32]) + 0.5)
    W[k0:k0 + 32] = _half_step_up((np.abs(W[k0:k0 + 32]) + np.float32(0.5 / math.sqrt(K))) * np.float32(2.0 * K))
    return slab


def _blocks128(N):
    return [slice(b, min(b + 128, N)) for b in range(0, N, 128)]


def gemm_operands(p):
    """The im2col operands of a pk_op_gemm problem and the scales the split kernel derives from them:
    -> Aim (M, K), Wim (K, N) float32 in the kernel's column order (natural; gate problems: as given, content | gate),
       sa (M, 1), sw (1, N)."""
    A, W = p["A"], p["W"]
    M, Cin, N = p["M"], p["Cin"], p["N"]
    if p.get("ntaps"):
        rows = [int(o) // p["lda"] for o in p["tap_off"][:p["ntaps"]]]
        tw = list(p["tap_w"][:p["ntaps"]])
    else:
        rows, tw = [t - p["pad"] for t in range(p["taps"])], list(range(p["taps"]))
    lo, hi = min(rows + [0]), max(rows + [0])
    Ap = np.zeros((M + hi - lo, Cin), np.float32)
    Ap[-lo:-lo + M] = A[:, :Cin]
    Aim = np.concatenate([Ap[-lo + o:-lo + o + M] for o in rows], axis=1)
    Wim = np.concatenate([W[t * Cin:(t + 1) * Cin] for t in tw], axis=0)
    own = np.abs(A[:, :Cin]).max(1) if p.get("a_amax") is None else np.asarray(p["a_amax"], np.float32)
    amp = np.zeros(M + hi - lo, np.float32)
    amp[-lo:-lo + M] = own
    blk = np.max([amp[-lo + o:-lo + o + M] for o in rows], axis=0)
    if p.get("Cin2"):
        A2 = p["A2"][:, :p["Cin2"]]
        Aim = np.concatenate([Aim, A2], axis=1)
        k0 = p["w2_slab0"] * 16
        Wim = np.concatenate([Wim, W[k0:k0 + p["Cin2"]]], axis=0)
        blk = np.maximum(blk, np.abs(A2).max(1) if p.get("a2_amax") is None else p["a2_amax"])
    sw = np.ones((1, N))
    if p.get("epi", 0) in (1, 2):                # gate: block nb = content and gate columns of channels 64 nb .. 64 nb + 63
        Cz = N // 2
        for b in range(0, Cz, 64):
            cols = np.r_[b:b + 64, Cz + b:Cz + b + 64]
            sw[0, cols] = fb.weight_scale(np.abs(W[:, cols]).max())
    else:
        for s in _blocks128(N):
            sw[0, s] = fb.weight_scale(np.abs(W[:, s]).max())
    return Aim, Wim, fb.act_scale(blk)[:, None], sw, own


def gemm_reference(p, split=True):
    """fp64 restatement of the formula in csrc/pk_gemm.h with the error propagated stage by stage ->
    dict(C, b_C [, C2, b_C2], pre, b_pre, Aim, Wim, sa, sw): C is (M, N) (gate: (M, N / 2)) BEFORE out_rowmap."""
    Aim, Wim, sa, sw, _ = gemm_operands(p)
    A64, W64 = Aim.astype(np.float64), Wim.astype(np.float64)
    M, N, K = p["M"], p["N"], Aim.shape[1]
    bias = np.zeros(N) if p.get("bias") is None else p["bias"].astype(np.float64)
    absprod = np.abs(A64) @ np.abs(W64)
    pre = A64 @ W64 + bias
    if split:
        b = fb.split_dot_bound(absprod, K, np.abs(A64).sum(1, keepdims=True), np.abs(W64).sum(0, keepdims=True), sa, sw,
                               bias)
    else:
        b = fb.dot_bound(absprod, K, bias)
    out = dict(pre=pre, b_pre=b, Aim=Aim, Wim=Wim, sa=sa, sw=sw, absprod=absprod)
    out.update(gemm_epilogue_reference(p, pre, b))
    return out


def gemm_epilogue_reference(p, pre, b, acc2=None):
    """the epilogue of gemm_reference from the product + bias `pre` with error `b` (tests/test_fp32_bounds_cpu.py feeds it
    emulated and mutated products) -> dict(C, b_C [, C2, b_C2]); acc2 overrides p["acc2"] (the overwritten-C2 mutant)"""
    M, N = p["M"], p["N"]
    acc2 = p.get("acc2") if acc2 is None else acc2
    out = {}
    gap = np.zeros(M, bool) if p.get("rowvalid") is None else p["rowvalid"] < 0
    epi = p.get("epi", 0)
    if epi in (1, 2):
        Cz = N // 2
        z = np.tanh(pre[:, :Cz]) / (1.0 + np.exp(-pre[:, Cz:]))
        bz = fb.gate_bound(pre[:, :Cz], pre[:, Cz:], b[:, :Cz], b[:, Cz:])
        z[gap], bz[gap] = 0.0, 0.0
        if epi == 1:
            out.update(C=z, b_C=bz)
            return out
        W2 = p["W2"].astype(np.float64)
        bias2 = np.zeros(128) if p.get("bias2") is None else p["bias2"].astype(np.float64)
        za = np.abs(z) + bz
        sw2 = np.full((1, 128), fb.weight_scale(np.abs(W2).max()))
        pre = z @ W2 + bias2
        b = bz @ np.abs(W2) + fb.split_dot_bound(za @ np.abs(W2), 64, za.sum(1, keepdims=True), np.abs(W2).sum(0, keepdims=True),
                                                 np.full((M, 1), 2.0 ** 14), sw2, bias2)
        N, act = 128, 0
    else:
        act = p.get("act", 0)
    res = None if p.get("res") is None else p["res"][:, :N].astype(np.float64)
    rp = p.get("res_pos", 0)
    v = pre
    if res is not None and rp == 2:
        v = v + res
        b = fb.epilogue_step(v, b)
    vact, bact = (np.maximum(pre, 0.0), b) if act == 1 else (np.tanh(pre), fb.tanh_bound(pre, b)) if act == 2 else (pre, b)
    if act == 1:
        v = np.maximum(v, 0.0)
    elif act == 2:
        v, b = np.tanh(v), fb.tanh_bound(v, b)
    cs = None if p.get("cscale") is None else p["cscale"].astype(np.float64)
    ch = np.zeros(N) if p.get("cshift") is None else p["cshift"].astype(np.float64)

    def affine(v, b):
        if cs is None:
            return v, b
        return v * cs + ch, fb.epilogue_step(v * cs + ch, np.abs(cs) * b + U_ * np.abs(v * cs))

    U_ = fb.U
    g2 = gap[:, None]
    if rp == 0:
        if res is not None:
            v = v + res
            b = fb.epilogue_step(v, b)
        v, b = np.where(g2, 0.0, v), np.where(g2, 0.0, b)
        v, b = affine(v, b)
    else:
        v, b = affine(v, b)
        if res is not None and rp == 1:
            v = v + res
            b = fb.epilogue_step(v, b)
        v, b = np.where(g2, 0.0, v), np.where(g2, 0.0, b)
    ns = p.get("nsplit", 0)
    if ns > 0:
        # columns >= nsplit: act(product + bias), no residual, no affine; + the old C2 where acc2; a gap row stores 0
        old = p["C2_old"][:, :N - ns].astype(np.float64) if acc2 else np.zeros((M, N - ns))
        v2 = vact[:, ns:] + old
        b2 = fb.epilogue_step(v2, bact[:, ns:]) if p.get("acc2") else bact[:, ns:]
        out.update(C2=np.where(g2, 0.0, v2), b_C2=np.where(g2, 0.0, b2))
        v, b = v[:, :ns], b[:, :ns]
    out.update(C=v, b_C=b)
    return out


# ------------------------------------------------------------------------------------------------ row GEMM (pk_op_rowgemm)
ROW_M, ROW_K, ROW_N = (1, 2, 31, 32), (4, 64, 508, 512, 516, 1024, 2560), (1, 15, 16, 17, 80, 1030)
RowCase = namedtuple("RowCase", "M K N bias")
# every (K, N) pair once; for a fixed N the seven K values walk through the four M values
ROW_CASES = [RowCase(ROW_M[(ki + ni) % 4], K, N, (ki + ni) % 2 == 0) for ni, N in enumerate(ROW_N) for ki, K in enumerate(ROW_K)]
ROW_LN_K = (64, 256, 512)
ROW_LSTM_H = (4, 16, 36, 256)


def row_id(c):
    return f"M{c.M}-K{c.K}-N{c.N}-{'bias' if c.bias else 'nobias'}"


def rowgemm_inputs(M, K, N, tag="row", bias=True):
    r = rng_for(tag, M, K, N)
    return (f32(r.normal(0.5, 1.0, (M, K))), f32(r.normal(0.3, 1.0, (K, N)) / math.sqrt(K)),
            f32(r.normal(0.2, 0.5, N)) if bias else None)


def layernorm_rows(M, K, tag="ln"):
    """rows for the LayerNorm prologue: ordinary ones, a constant row (variance 0) and one whose mean is 16 spreads"""
    r = rng_for(tag, M, K)
    x = f32(r.normal(0.5, 1.0, (M, K)))
    x[0] = 3.0
    if M > 1:
        x[1] += 16.0
    return x, f32(r.uniform(0.5, 1.5, K)), f32(r.normal(0.3, 0.5, K))


def rowgemm_ln_reference(x, g, beta, w, bias, eps=1e-5):
    xn, b_xn = fb.layernorm_bound(x, g, beta, np.float32(eps))
    W = np.asarray(w, np.float64)
    b = np.zeros(W.shape[1]) if bias is None else np.asarray(bias, np.float64)
    absW = np.abs(W)
    return xn @ W + b, b_xn @ absW + fb.dot_bound((np.abs(xn) + b_xn) @ absW, x.shape[1], b), xn, b_xn


def lstm_reference(x, w, bias, c, b_c=0.0):
    """one LSTMCell step on gate columns [i | f | g | o] -> (c', h, b_c', b_h)"""
    H = w.shape[1] // 4
    pre, b_pre = matmul_reference(x, w, bias)
    b_gate = np.maximum.reduce([b_pre[:, i * H:(i + 1) * H] for i in range(4)])      # one bound for the unit's four gates
    return fb.lstm_bound(pre[:, :H], pre[:, H:2 * H], pre[:, 2 * H:3 * H], pre[:, 3 * H:], b_gate, c, b_c)


# ---- the problems of the feature tests (gate, projection, nsplit, A2, skipped tap, mixed magnitudes, given row maxima):
# built here so that tests/test_fp32_bounds_cpu.py proves on the host that the bound sees a wrong kernel on these inputs
def _gap_vector(M):
    rv = np.zeros(M, np.int32)
    rv[gemm_gap_rows(M)] = -1
    return rv


def _conv_problem(tag, M, N, Cin, taps, loud=-1, scale=1.0, **kw):
    r = rng_for("gemmx", tag, M, N, Cin, taps)
    K = taps * Cin
    p = dict(M=M, N=N, Cin=Cin, taps=taps, pad=(taps - 1) // 2, lda=Cin, A=f32(r.normal(0.5, 1.0, (M, Cin))),
             W=f32(r.normal(0.3, 1.0, (K, N)) / math.sqrt(K)))
    p["loud"] = gemm_loud_slab(p["A"], p["W"], Cin, K, loud)
    p["W"] = f32(p["W"] * np.float32(scale))
    p.update(kw)
    return p, r


def gate_problem(N, bias, proj=False):
    """pre-activations of order 1 (the loud slab is one-signed: scaled down by a power of two so that tanh and sigmoid stay
    in their steep part, where a wrong product is not hidden by saturation)"""
    M = 150 if proj else 129
    p, r = _conv_problem(("gate", N, bias, proj), M, N, 64, 3, scale=2.0 ** -15, epi=2 if proj else 1, rowvalid=_gap_vector(M))
    if bias:
        p["bias"] = f32(r.normal(0.0, 0.1, N))
    if proj:
        p.update(W2=f32(r.normal(0.3, 1, (64, 128)) / 8), bias2=f32(r.normal(0.2, 0.5, 128)), res=f32(r.normal(0.3, 1, (M, 128))),
                 ldr=128)
    return p


def nsplit_problem(nsplit, acc2):
    p, r = _conv_problem("nsplit", 129, 192, 64, 3, bias=None, act=1, rowvalid=_gap_vector(129), nsplit=nsplit, acc2=acc2)
    p.update(bias=f32(r.normal(0.2, 0.5, 192)), res=f32(r.normal(0.3, 1, (129, 195))), ldr=195,
             C2_old=f32(rng_for("c2").normal(0.3, 1, (129, 192 - nsplit)) * 4096))
    return p


GEMM_A2_SHAPES = ((32, 32), (64, 32), (64, 96))     # (Cin, Cin2) at 3 taps: 4, 7 and 9 K slabs


def a2_problem(Cin, Cin2, loud, explicit=True):
    """loud: K slab index; the last Cin2 / 32 slabs lie in the A2 block"""
    M, N, taps = 129, 129, 3
    r = rng_for("a2", Cin, Cin2, loud)
    K = taps * Cin + Cin2
    p = dict(M=M, N=N, Cin=Cin, lda=Cin, A=f32(r.normal(0.5, 1, (M, Cin))), A2=f32(r.normal(0.2, 3, (M, Cin2 + 4))), lda2=Cin2 + 4,
             Cin2=Cin2, w2_slab0=taps * Cin // 16, W=f32(r.normal(0.3, 1, (K, N)) / math.sqrt(K)), bias=f32(r.normal(0.2, 0.5, N)))
    if explicit:
        p.update(ntaps=taps, wtaps=taps, tap_off=[(t - 1) * Cin for t in range(taps)], tap_w=list(range(taps)))
    else:
        p.update(taps=taps, pad=1)
    p["loud"] = gemm_loud_slab(p["A"], p["W"], Cin, K, loud, p["A2"], taps * Cin)
    return p


def skipped_tap_problem():
    """5 packed taps of which tap 2 (the row itself) is skipped through tap_w = [0, 1, 3, 4]: 4 K slabs at Cin = 32.  Odd rows
    of A are zero, so on odd output rows the skipped tap reads zeros and the full convolution must give the same bits."""
    M, Cin, N = 130, 32, 129
    r = rng_for("skip")
    A = f32(r.normal(0.5, 1, (M, Cin)))
    A[1::2] = 0
    W = f32(r.normal(0.3, 1, (5 * Cin, N)) / math.sqrt(5 * Cin))
    full = dict(M=M, N=N, Cin=Cin, lda=Cin, A=A, W=W, taps=5, pad=2)
    part = dict(M=M, N=N, Cin=Cin, lda=Cin, A=A, W=W, ntaps=4, wtaps=5, tap_off=[(t - 2) * Cin for t in (0, 1, 3, 4)],
                tap_w=[0, 1, 3, 4])
    # im2col slab 1 of `part` = tap 1 = weight rows 32..63 of both; the weight rows of tap 3 differ from those of tap 2
    part["loud"] = gemm_loud_slab(A, W, Cin, 4 * Cin, 1)
    A[1::2] = 0
    return full, part


def mixed_problem(taps):
    M, N, Cin = 385, 129, 64
    p, r = _conv_problem(("mixed", taps), M, N, Cin, taps)
    A = p["A"]
    A[0:40:2] *= np.float32(2.0 ** 12)            # neighbours 2^12 apart: a row scaled by its own maximum alone overflows fp16
    A[41:80:2] *= np.float32(2.0 ** -12)
    A[90, 7] *= np.float32(2.0 ** 20)             # one element 2^20 above its row
    A[100:110] = 0                                # zero rows inside live ones
    A[128:256] = 0                                # a whole zero 128-row tile (two 64-row tiles)
    A[300:310] = f32(r.choice([-1, 1], (10, Cin))) * np.float32(2.0 ** -41)   # below the clamp of the block exponent
    A[296:300] = 0
    A[310:314] = 0
    return p


def amax_problem(factor):
    p, _ = _conv_problem("amax", 129, 129, 64, 3)
    if factor:
        p["a_amax"] = f32(factor * np.abs(p["A"]).max(1))
    return p


GEMM_FEATURE_PROBLEMS = (
    [(f"gate-N{N}-{'bias' if b else 'nobias'}", lambda N=N, b=b: gate_problem(N, b)) for N in (128, 256) for b in (False, True)] +
    [("gateproj", lambda: gate_problem(128, True, True))] +
    [(f"nsplit{ns}-acc{a}", lambda ns=ns, a=a: nsplit_problem(ns, a)) for ns in (64, 128) for a in (0, 1)] +
    [(f"a2-Cin{ci}-Cin2_{c2}-loud{sl}", lambda ci=ci, c2=c2, sl=sl: a2_problem(ci, c2, sl))
     for ci, c2 in GEMM_A2_SHAPES for sl in sorted({0, (3 * ci + c2) // 64, 3 * ci // 32, (3 * ci + c2) // 32 - 1})] +
    [("a2-tapspad", lambda: a2_problem(64, 32, 6, explicit=False))] +
    [("skipped-tap", lambda: skipped_tap_problem()[1])] +
    [(f"mixed-k{t}", lambda t=t: mixed_problem(t)) for t in (3, 5)] +
    [("amax-x2", lambda: amax_problem(2.0))])


def stop_inputs(ln):
    """6 rows, K = 256, whose stop logit is far from 0: rows 0, 2, 4 above, rows 1, 3, 5 below.  Without LayerNorm the rows are
    moved along the stop vector to +-6; under LayerNorm (which undoes such a shift) the stop vector is built from the
    normalised rows instead: a combination of them that has the wanted sign pattern."""
    M, K = 6, 256
    r = rng_for("stop", ln)
    x = f32(r.normal(0.5, 1.0, (M, K)))
    target = np.where(np.arange(M) % 2 == 0, 6.0, -6.0)
    if not ln:
        sw = f32(r.normal(0, 1, K) / math.sqrt(K))
        s64 = sw.astype(np.float64)
        x = f32(x + ((target - x.astype(np.float64) @ s64) / (s64 @ s64))[:, None] * s64)
        return x, sw, None, None
    g, beta = f32(r.uniform(0.5, 1.5, K)), f32(r.normal(0, 0.3, K))
    xn, _ = fb.layernorm_bound(x, g, beta, np.float32(1e-5))
    sw = f32(np.linalg.lstsq(xn, target, rcond=None)[0])          # minimum-norm solution of xn . sw = target
    return x, sw, g, beta


def stop_reference(x, sw, g, beta, sbias):
    """-> (logit, bound, the rows the dot product sees)"""
    ln = g is not None
    xn, b_xn = fb.layernorm_bound(x, g, beta, np.float32(1e-5)) if ln else (x.astype(np.float64), np.zeros(x.shape))
    s64 = sw.astype(np.float64)
    logit = xn @ s64 + sbias
    b = b_xn @ np.abs(s64) + fb.dot_bound((np.abs(xn) + b_xn) @ np.abs(s64), x.shape[1], np.full(x.shape[0], abs(sbias)))
    return logit, b, xn
