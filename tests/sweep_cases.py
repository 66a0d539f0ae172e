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
