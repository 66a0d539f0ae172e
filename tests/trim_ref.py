"""Silence trimming restated in numpy float64, the bounds the tests use and their signals (a plain module, not
a conftest).  Nothing here imports parakeet_amd.

    frames  = 1 + (N + 2 (Lf // 2) - Lf) // hop centred, 1 + (N - Lf) // hop (0 for N < Lf) otherwise
    P[i]    = (1 / Lf) sum_{j < Lf} x~[i hop - pad + j]^2, x~ = numpy's reflect (or zero) continuation of the utterance
    frame i is non-silent iff 10 log10(max(a, P[i])) - 10 log10(max(a, max P)) > -top_db, a = 1e-10   (librosa 0.8, ref=np.max)
    trim    = (first non-silent frame * hop, min(N, (last + 1) * hop)), (0, 0) without one;  split = the runs, the same way
    trim_long_silences: windows of w samples, flags -> c = flags in [k - (W - 1) // 2, k + W // 2] -> mask = 2 c > W ->
    keep[k] = any mask[k - (L - 1 - L // 2) ... k + L // 2], L = S + 1 -> the samples of the kept windows
    energy detector (this project's, NOT webrtcvad): flag[k] iff Q[k] > max(max Q * 10^(-vad_top_db / 10), 10^(vad_floor_dBFS / 10))

The error bound of P.  csrc/pk_trim.h states the order: lane l sums x_j^2 over j = l, l + 64, ... with one FMA each (the product
is not rounded: one rounding per step, at most ceil(Lf / 64) of them on any term), the 64 lane sums meet in a six-level
butterfly (six additions on any term), one division by Lf.  Every term is >= 0, so each rounding is a relative perturbation
of the partial sum it lands on and of every term inside it: a term x_j^2 reaches P multiplied by at most
(1 + u)^(ceil(Lf / 64) + 7), hence |P - P_exact| <= ((ceil(Lf / 64) + 7) u) P_exact to first order -- relative, never above the
(Lf + 2) u that holds for ANY order of Lf FMAs and a division.  ``eps_P`` carries 0.1 % for the second-order terms.
"""
import math

import numpy as np

U = 2.0 ** -24
AMIN = 1e-10
FLT_MIN = float(np.finfo(np.float32).tiny)


# ---- definitions
def num_frames(n, Lf, hop, center=True):
    padded = n + (2 * (Lf // 2) if center else 0)
    return 0 if padded < Lf else 1 + (padded - Lf) // hop


def frame_power(x, Lf=2048, hop=512, center=True, pad_mode="reflect"):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if center:
        if pad_mode == "reflect" and x.size <= Lf // 2:
            raise ValueError("reflect padding needs more than Lf // 2 samples")
        x = np.pad(x, Lf // 2, mode=pad_mode)
    nf = num_frames(x.size, Lf, hop, False)
    if nf == 0:
        return np.zeros(0)
    X = np.lib.stride_tricks.as_strided(x, shape=(nf, Lf), strides=(hop * x.strides[0], x.strides[0]))
    return np.einsum("ij,ij->i", X, X) / Lf


def nonsilent(P, top_db):
    """the frame test in decibels, as librosa writes it"""
    P = np.asarray(P, dtype=np.float64)
    if P.size == 0:
        return np.zeros(0, bool)
    db = 10.0 * np.log10(np.maximum(AMIN, P)) - 10.0 * np.log10(max(AMIN, P.max()))
    return db > -top_db


def decided_frames(P, top_db, eps):
    """where the linear form max(a, P[i]) > max(a, Pmax) 10^(-top_db / 10) keeps its side when P[i] and Pmax each move by the
    relative eps: the distance from the threshold exceeds the bound on both sides"""
    P = np.asarray(P, dtype=np.float64)
    if P.size == 0:
        return np.zeros(0, bool)
    v = np.maximum(AMIN, P)
    t = max(AMIN, P.max()) * 10.0 ** (-top_db / 10.0)
    return np.abs(v - t) > eps * (v + t)


def runs(flags):
    """(n, 2) [first, last + 1) of every run of set flags"""
    f = np.concatenate([[0], np.asarray(flags).astype(np.int8), [0]])
    return np.flatnonzero(np.diff(f)).reshape(-1, 2)


def trim_index(x, top_db=60, Lf=2048, hop=512, pad_mode="reflect"):
    n = np.asarray(x).size
    nz = np.flatnonzero(nonsilent(frame_power(x, Lf, hop, True, pad_mode), top_db))
    if nz.size == 0:
        return np.array([0, 0], np.int64)
    return np.array([nz[0] * hop, min(n, (nz[-1] + 1) * hop)], np.int64)


def split_index(x, top_db=60, Lf=2048, hop=512, pad_mode="reflect"):
    n = np.asarray(x).size
    return np.minimum(runs(nonsilent(frame_power(x, Lf, hop, True, pad_mode), top_db)).astype(np.int64) * hop, n)


def peak_normalize(y):
    """float32 numpy: one division per sample"""
    y = np.asarray(y, dtype=np.float32)
    m = np.abs(y).max()
    return y.copy() if m < np.float32(FLT_MIN) else y / m


def smooth(flags, W):
    """mask[k] iff 2 c > W, c = the set flags in [k - (W - 1) // 2, k + W // 2] inside the array"""
    f = np.asarray(flags).astype(np.int64)
    return 2 * _count(f, (W - 1) // 2, W // 2) > W


def _count(f, lo, hi):
    cs = np.concatenate([[0], np.cumsum(f)])
    k = np.arange(f.size)
    return cs[np.minimum(f.size, k + hi + 1)] - cs[np.maximum(0, k - lo)]


def moving_average_rounded(flags, W):
    """The reference's own arithmetic (audio_processor.py:92-100), restated: the flags between (W - 1) // 2 leading and W // 2
    trailing zeros, a running sum, the difference of the sum W apart, / W, np.round (half to even), as booleans."""
    a = np.concatenate([np.zeros((W - 1) // 2), np.asarray(flags, dtype=np.float64), np.zeros(W // 2)])
    s = np.cumsum(a, dtype=float)
    s[W:] = s[W:] - s[:-W]
    return np.round(s[W - 1:] / W).astype(bool)


def dilate(mask, S):
    """keep[k] = any mask[k - (L - 1 - L // 2) ... k + L // 2], L = S + 1"""
    m = np.asarray(mask).astype(bool)
    L = S + 1
    lo, hi = L - 1 - L // 2, L // 2
    return np.array([m[max(0, k - lo):k + hi + 1].any() for k in range(m.size)], bool)


def window_size(vad_window_length, sampling_rate):
    return (vad_window_length * sampling_rate) // 1000


def keep_mask(flags, W, S):
    return dilate(smooth(flags, W), S)


def trim_long_silences(wav, flags, w, W, S):
    wav = np.asarray(wav)
    n_w = wav.size // w
    flags = np.asarray(flags).astype(bool)
    assert flags.size == n_w
    return wav[:n_w * w][np.repeat(keep_mask(flags, W, S), w)]


def window_power(x, w):
    return frame_power(x, w, w, center=False)


def energy_flags(x, w, vad_top_db=40, vad_floor_dBFS=-50):
    """-> (Q, flags, threshold)"""
    Q = window_power(x, w)
    if Q.size == 0:
        return Q, np.zeros(0, bool), 0.0
    thr = max(Q.max() * 10.0 ** (-vad_top_db / 10.0), 10.0 ** (vad_floor_dBFS / 10.0))
    return Q, Q > thr, thr


def decided_windows(Q, thr, eps):
    """a window is decided when Q[k] and the threshold (which moves with max Q by at most eps, if at all) keep their sides"""
    return np.abs(np.asarray(Q) - thr) > eps * (np.asarray(Q) + thr)


def vad_golden(path):
    """tests/golden/vad_post.npz (tools/make_golden_vad.py) -> a list of dicts: name, wav, flags, out and the reference's
    arguments ms (window), W, S, sr"""
    g = np.load(path)
    wo = np.concatenate([[0], np.cumsum(g["wav_len"])])
    oo = np.concatenate([[0], np.cumsum(g["out_len"])])
    cases, fo = [], 0
    for i, name in enumerate(g["names"]):
        ms, W, S, sr = (int(v) for v in g["params"][i])
        wav = g["wav"][wo[i]:wo[i + 1]]
        n_w = wav.size // window_size(ms, sr)
        cases.append(dict(name=str(name), wav=wav, flags=g["flags"][fo:fo + n_w], out=g["out"][oo[i]:oo[i + 1]], ms=ms, W=W, S=S,
                          sr=sr))
        fo += n_w
    assert fo == g["flags"].size
    return cases


# ---- bounds
def eps_P(Lf):
    return 1.001 * (math.ceil(Lf / 64) + 7) * U


def eps_any_order(Lf):
    return 1.001 * (Lf + 2) * U


def emulate_power_f32(x, Lf, hop, center=True, pad_mode="reflect"):
    """The kernel's order in numpy float32 (the FMA as a float64 product and sum rounded once: exact products, and a sum of a
    24-bit and a 48-bit number is rounded to float32 from a float64 that holds it to 53 bits -- a double rounding in rare
    cases, which this CPU sanity check of the bound tolerates)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if center:
        x = np.pad(x, Lf // 2, mode=pad_mode)
    nf = num_frames(x.size, Lf, hop, False)
    out = np.zeros(nf, np.float32)
    for i in range(nf):
        fr = x[i * hop:i * hop + Lf].astype(np.float64)
        s = np.zeros(64, np.float32)
        for j0 in range(0, Lf, 64):
            blk = fr[j0:j0 + 64]
            s[:blk.size] = (blk * blk + s[:blk.size].astype(np.float64)).astype(np.float32)
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[np.arange(64) ^ off]
        out[i] = s[0] / np.float32(Lf)
    return out


# ---- signals
def tone(n, sr=24000, f=220.0, amp=0.3, phase=0.0):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / sr + phase)).astype(np.float32)


def trim_cases():
    """name -> float32 signal for the trim / split / flag tests at (Lf, hop) = (2048, 512), top_db 20 and 60.  Silence is a
    1e-5 noise floor (-100 dB: far from both thresholds), sound a 0.3 tone with 1 % noise; the edges are hard, so only the
    frames that straddle an edge sit between the two levels, and the CPU test asserts that none of them is undecided."""
    rng = np.random.default_rng(7)

    def sil(n):
        return (1e-5 * rng.standard_normal(n)).astype(np.float32)

    def snd(n):
        return tone(n, phase=rng.uniform(0, 6.28)) + (3e-3 * rng.standard_normal(n)).astype(np.float32)
    impulse = np.zeros(9000, np.float32)
    impulse[4321] = 0.5
    return {
        "lead_trail": np.concatenate([sil(3333), snd(7001), sil(2777)]),
        "to_last_sample": np.concatenate([sil(1900), snd(6100 + 255)]),
        "from_first_sample": np.concatenate([snd(5000), sil(4100)]),
        "impulse": impulse,
        "zeros": np.zeros(6000, np.float32),
        "bursts": np.concatenate([sil(2100), snd(3000), sil(4999), snd(2500), sil(3100), snd(4000), sil(1234)]),
        "all_sound": snd(7777),
    }


GE2E = dict(sampling_rate=16000, vad_window_length=30, vad_moving_average_width=8, vad_max_silence_length=6)


def burst_signal(gaps=(6, 9, 14, 25), burst=12, lead=3, trail=4, seed=0, sr=16000, w=480):
    """Tone bursts of ``burst`` windows separated by silences of ``gaps`` windows over a 1e-3 noise floor, window-aligned, plus
    a tail of w // 3 samples that trim_long_silences drops.  -> (float32 signal, the voice flags by construction)."""
    rng = np.random.default_rng(seed)
    flags = [0] * lead
    for g in gaps:
        flags += [1] * burst + [0] * g
    flags += [1] * burst + [0] * trail
    flags = np.array(flags, bool)
    n = flags.size * w + w // 3
    x = 1e-3 * rng.standard_normal(n)
    env = np.concatenate([np.repeat(flags, w), np.zeros(w // 3, bool)])
    x = x + env * 0.3 * np.sin(2 * np.pi * 180.0 * np.arange(n) / sr)
    return x.astype(np.float32), flags


def pause_signal():
    """6.7 s at 16 kHz with a pause of 2.4 s: the GE2E front end cuts fewer partials from it once the pause is shortened"""
    return burst_signal(gaps=(6, 80, 9), burst=30, seed=5)
