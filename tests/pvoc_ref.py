"""The phase vocoder of csrc/pk_pvoc.h restated in float64 numpy, operation by operation: THE DEFINITION the
engine must equal bit for bit.  Every product, sum, root and quotient below is one numpy ufunc call on float64 arrays -- one
IEEE operation per element, no fused multiply-add, no complex arithmetic, no transcendental function.  Change the header,
change this file.

Also here, for the tests: the LITERAL formula of librosa 0.8's ``phase_vocoder`` (angle, wrap, cumulative sum) and a numpy
model of STFT -> phase vocoder -> ISTFT for the sine checks (librosa is not installed; both are written out from its source as
published)."""
import math

import numpy as np

THREADS = 64            # PVOC_THREADS: bins per workgroup
AHEAD = 4               # PVOC_AHEAD
MAX_BATCH = 65535       # PVOC_MAX_BATCH
MAX_FRAMES = 1 << 31    # PVOC_MAX_FRAMES: T stays below


def num_frames(F, rate):
    """T = ceil((double)F / rate)."""
    return int(math.ceil(float(F) / float(rate)))


def _polar(re, im):
    """m(z), u(z): float64 arrays in, (m, ur, ui) out; u = (1, 0) where m == 0."""
    m = np.sqrt(re * re + im * im)
    nz = m > 0.0
    d = np.where(nz, m, 1.0)
    return m, np.where(nz, re / d, 1.0), np.where(nz, im / d, 0.0)


def phase_vocoder_rows64(rows, rate):
    """rows: (F, 2 * n_bin) float32 re | im -> (T, 2 * n_bin) float64: the products mag_t * p_t BEFORE their one rounding to
    float32.  The bins are independent; numpy runs them side by side."""
    rows = np.asarray(rows, dtype=np.float32)
    F, nb = rows.shape[0], rows.shape[1] // 2
    rate = float(rate)
    T = num_frames(F, rate)
    re = np.zeros((F + 2, nb), np.float64)        # rows at or beyond F read as zero (k_t <= F: see csrc/pvoc.hip's clamp)
    im = np.zeros((F + 2, nb), np.float64)
    re[:F], im[:F] = rows[:, :nb], rows[:, nb:]
    out = np.empty((T, 2 * nb), np.float64)
    _, pr, pi = _polar(re[0], im[0])
    for t in range(T):
        step = float(t) * rate
        kf = math.floor(step)
        k = int(kf)
        al = step - float(kf)
        k0, k1 = min(k, F), min(k + 1, F + 1)     # any row >= F is a zero row
        m0, a, b = _polar(re[k0], im[k0])
        m1, c, d = _polar(re[k1], im[k1])
        mag = (1.0 - al) * m0 + al * m1
        out[t, :nb] = mag * pr
        out[t, nb:] = mag * pi
        wr, wi = c * a + d * b, d * a - c * b
        qr, qi = pr * wr - pi * wi, pr * wi + pi * wr
        mq = np.sqrt(qr * qr + qi * qi)
        pr, pi = qr / mq, qi / mq
    return out


def phase_vocoder_rows(rows, rate):
    """rows: (F, 2 * n_bin) float32 re | im -> (T, 2 * n_bin) float32: the engine's output, bit for bit."""
    return phase_vocoder_rows64(rows, rate).astype(np.float32)


def to_rows(D):
    """complex (n_bin, F) -> (F, 2 * n_bin) float32 re | im."""
    D = np.asarray(D)
    return np.ascontiguousarray(np.concatenate([D.real.T, D.imag.T], axis=1), dtype=np.float32)


def from_rows(rows):
    """(T, 2 * n_bin) -> complex (n_bin, T)."""
    nb = rows.shape[1] // 2
    return (rows[:, :nb].astype(np.float64) + 1j * rows[:, nb:].astype(np.float64)).T


def phase_vocoder(D, rate):
    """librosa's shape: complex (n_bin, F) -> complex128 (n_bin, T) holding the float32 values of the definition."""
    return from_rows(phase_vocoder_rows(to_rows(D), rate))


def literal_phase_vocoder(D, rate, hop_length):
    """librosa 0.8 ``core.phase_vocoder`` as published, in float64 / complex128: for the comparison, not the definition."""
    D = np.asarray(D, dtype=np.complex128)
    time_steps = np.arange(0, D.shape[1], rate, dtype=np.float64)
    d_stretch = np.zeros((D.shape[0], len(time_steps)), np.complex128)
    phi_advance = np.linspace(0, np.pi * hop_length, D.shape[0])
    phase_acc = np.angle(D[:, 0])
    D = np.pad(D, [(0, 0), (0, 2)], mode="constant")
    for t, step in enumerate(time_steps):
        columns = D[:, int(step):int(step + 2)]
        alpha = np.mod(step, 1.0)
        mag = (1.0 - alpha) * np.abs(columns[:, 0]) + alpha * np.abs(columns[:, 1])
        d_stretch[:, t] = mag * np.exp(1.0j * phase_acc)
        dphase = np.angle(columns[:, 1]) - np.angle(columns[:, 0]) - phi_advance
        dphase = dphase - 2.0 * np.pi * np.round(dphase / (2.0 * np.pi))
        phase_acc += phi_advance + dphase
    return d_stretch


# ----------------------------------------------------------------- a numpy model of the whole effect (the sine checks)
def _hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def stft_model(y, n_fft, hop):
    """librosa's ``stft`` with a periodic Hann window, center=True, reflect padding: complex (n_bin, 1 + len(y) // hop)."""
    y = np.pad(np.asarray(y, np.float64), n_fft // 2, mode="reflect")
    n = 1 + (len(y) - n_fft) // hop
    w = _hann(n_fft)
    return np.stack([np.fft.rfft(w * y[i * hop:i * hop + n_fft]) for i in range(n)], axis=1)


def istft_model(D, n_fft, hop, length):
    """librosa's ``istft``: windowed overlap-add divided by the summed squared window, the centre padding removed, cropped or
    zero-padded to ``length``."""
    T = D.shape[1]
    w = _hann(n_fft)
    y = np.zeros(n_fft + hop * (T - 1))
    ws = np.zeros_like(y)
    for i in range(T):
        y[i * hop:i * hop + n_fft] += w * np.fft.irfft(D[:, i], n_fft)
        ws[i * hop:i * hop + n_fft] += w * w
    nz = ws > np.finfo(np.float32).tiny
    y[nz] /= ws[nz]
    y = y[n_fft // 2:]
    return y[:length] if len(y) >= length else np.pad(y, (0, length - len(y)))


def time_stretch_model(y, rate, n_fft, hop):
    D = phase_vocoder(stft_model(y, n_fft, hop).astype(np.complex64), rate)
    return istft_model(D, n_fft, hop, int(round(len(y) / rate)))


def peak_hz(y, sr):
    """The frequency of the largest bin of the Hann-windowed middle half of y, refined by a parabola through its neighbours."""
    y = np.asarray(y, np.float64)
    n = len(y)
    seg = y[n // 4:n - n // 4]
    s = np.abs(np.fft.rfft(seg * np.hanning(len(seg))))
    i = int(np.argmax(s[1:-1])) + 1
    a, b, c = np.log(s[i - 1] + 1e-300), np.log(s[i] + 1e-300), np.log(s[i + 1] + 1e-300)
    off = 0.5 * (a - c) / (a - 2 * b + c)
    return (i + off) * sr / len(seg)
