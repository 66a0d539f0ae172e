"""STFT / mel features behind the reference's Python API.

Mirrors parakeet/modules/audio.py ``STFT`` (:74-215: forward / power / magnitude) and ``MelScale``
(:218-229), and the host feature extractor ``LogMelFBank`` of parakeet/data/get_feats.py (:20-88);
the arithmetic (reflect padding, DFT-as-GEMM, magnitude, mel GEMM, log) runs in libpk_synth.so
(csrc/mel.hip).  The window and the mel filterbank are host-side constants handed to the engine;
``mel_filterbank`` follows the algorithm of librosa.filters.mel (Slaney scale and normalisation),
which the reference calls at audio.py:221 / get_feats.py:49-55.

The way back -- ``ISTFT``, ``AudioProcessor.stft`` / ``istft`` / ``griffin_lim`` / ``mel_to_linear`` and the weight-free
``GriffinLim`` vocoder -- follows parakeet/audio/audio.py:75-93 (librosa's ``istft``) and ``librosa.griffinlim``; it runs in
csrc/istft.hip.

``rfft`` / ``irfft``: the radix FFT of csrc/rfft.hip as a primitive.  ``transform="fft"`` on ``STFT``, ``ISTFT``,
``LogMelFBank`` and ``AudioProcessor`` (and through it ``GriffinLim``) runs their frames on it instead of the dense DFT
products (the default, ``"dense"``); it needs an n_fft that is a power of two from 32 to 4096.

``resample_filter`` / ``Resample`` / ``resample`` / ``load_wav`` put audio of any rate on the model's rate: a polyphase
Kaiser-windowed sinc defined in DESIGN.md 4.5d (this project's own filter; the reference calls ``librosa.load(path, sr=fs)``,
whose resampler is not available here and is not reproduced), run by csrc/resample.hip.

``Pitch`` / ``pitch_lags`` / ``continuous_f0_batch``: the reference's ``Pitch`` interface (get_feats.py:91-164) over this
project's own f0 estimator (csrc/pitch.hip; NOT pyworld's DIO + StoneMask) and the reference's continuous-f0,
log and token-average steps.

``sosfilt`` / ``lfilter`` / ``preemphasis`` / ``deemphasis``: recursive filters as cascades of second-order sections in float64
(csrc/iir.hip), ``k_weighting`` and ``normalize_loudness``: gated programme loudness after ITU-R BS.1770-4 as
this project restates it for mono (NOT pyloudnorm, NOT libebur128; blocks on a 100 ms sample grid, ``sr % 10 == 0``).

``phase_vocoder`` / ``time_stretch`` / ``pitch_shift`` (and their ``_batch`` forms): the two effects of ``librosa.effects`` the
set lacked, over librosa 0.8's phase vocoder as this project restates it without any transcendental function (DESIGN.md 4.5i,
csrc/pvoc.hip; no phase locking; ``pitch_shift`` resamples with this project's filter at a rational ratio).
"""
import ctypes as C
import math
import struct
from fractions import Fraction

import numpy as np
import scipy.signal
import torch

from . import _capi
from .runtime import Context, dptr, wrap


def _slaney_hz(m):
    f_sp, brk_mel, step = 200.0 / 3.0, 15.0, math.log(6.4) / 27.0
    m = np.asarray(m, dtype=np.float64)
    lin = m * f_sp
    return np.where(m >= brk_mel, 1000.0 * np.exp(step * (m - brk_mel)), lin)


def _slaney_mel(f):
    f_sp, brk_mel, step = 200.0 / 3.0, 15.0, math.log(6.4) / 27.0
    return f / f_sp if f < 1000.0 else brk_mel + math.log(f / 1000.0) / step


def mel_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """Triangular Slaney-normalised mel filters, (n_mels, 1 + n_fft//2) float32."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    freqs = np.arange(1 + n_fft // 2, dtype=np.float64) * (sr / 2.0) / (n_fft // 2)
    edges = _slaney_hz(np.linspace(_slaney_mel(float(fmin)), _slaney_mel(fmax), n_mels + 2))
    lo, mid, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    up = (freqs[None, :] - lo) / (mid - lo)
    down = (hi - freqs[None, :]) / (hi - mid)
    tri = np.clip(np.minimum(up, down), 0.0, None)
    return (tri * (2.0 / (hi - lo))).astype(np.float32)


def _window(window, win_length, n_fft):
    name = "hann" if window == "hanning" else window
    w = scipy.signal.get_window(name, win_length, fftbins=True)
    if n_fft != win_length:
        left = (n_fft - win_length) // 2
        w = np.pad(w, (left, n_fft - win_length - left))
    return np.ascontiguousarray(w, dtype=np.float32)


def _transform_id(transform):
    if transform not in _capi.PK_TRANSFORM:
        raise ValueError(f"transform must be 'dense' or 'fft', got {transform!r}")
    return _capi.PK_TRANSFORM[transform]


def rfft_supported(n):
    """True where the radix FFT takes n points: a power of two from 32 to 4096."""
    return bool(_capi.lib().pk_rfft_supported(int(n)))


def rfft_tile_rows(n):
    """Rows one workgroup of the FFT kernels transforms at n points."""
    r = C.c_int32()
    _capi.check(_capi.lib().pk_rfft_tile_rows(int(n), C.byref(r)))
    return r.value


def rfft(x, as_complex=False, device=None):
    """``numpy.fft.rfft`` of the rows of x (rows, n) on the engine's radix FFT (csrc/rfft.hip), n a power of two from 32 to
    4096.  Returns a (rows, n + 2) device tensor re | im per row, the layout of ``pk_mel_run(what=0)``; with
    ``as_complex`` a complex64 (rows, n/2 + 1) tensor."""
    ctx = Context.get(device)
    x = ctx.to_device(x)
    if x.dim() != 2:
        raise AssertionError(f"rfft: expected (rows, n), got {tuple(x.shape)}")
    x = x.contiguous()
    rows, n = x.shape
    out = ctx.empty((rows, n + 2))
    _capi.check(ctx.lib.pk_op_rfft(ctx.handle, dptr(x), rows, n, dptr(out)))
    if as_complex:
        return wrap(torch.complex(out[:, :n // 2 + 1], out[:, n // 2 + 1:]))
    return wrap(out)


def irfft(spec, n=None, device=None):
    """``numpy.fft.irfft`` of the rows of spec: (rows, n + 2) re | im or complex (rows, n/2 + 1) -> (rows, n) device tensor.
    The imaginary parts of DC and Nyquist are ignored.  ``n`` may be given to check it; it follows from the shape."""
    ctx = Context.get(device)
    if isinstance(spec, np.ndarray) and np.iscomplexobj(spec):
        spec = np.concatenate([spec.real, spec.imag], axis=1).astype(np.float32)
    elif isinstance(spec, torch.Tensor) and spec.is_complex():
        spec = torch.cat([spec.real, spec.imag], dim=1).to(torch.float32)
    spec = ctx.to_device(spec)
    if spec.dim() != 2 or spec.shape[1] < 4 or spec.shape[1] % 2:
        raise AssertionError(f"irfft: expected (rows, n + 2) re | im or complex (rows, n/2 + 1), got {tuple(spec.shape)}")
    spec = spec.contiguous()
    rows, m = spec.shape[0], spec.shape[1] - 2
    if n is not None and int(n) != m:
        raise AssertionError(f"irfft: the rows hold the spectrum of {m} points, n = {n} was asked for")
    out = ctx.empty((rows, m))
    _capi.check(ctx.lib.pk_op_irfft(ctx.handle, dptr(spec), rows, m, dptr(out)))
    return wrap(out)


class _Engine:
    def __init__(self, n_fft, hop_length, win_length, window, center, power, mel_basis, log_base, device=None,
                 transform="dense"):
        tid = _transform_id(transform)
        self.transform = transform
        self.ctx = Context.get(device)
        cfg = _capi.MelCfg(n_fft, hop_length, 1 if center else 0, 1 if power else 0,
                           0 if mel_basis is None else mel_basis.shape[0], log_base, 1e-10)
        self.n_bin = 1 + n_fft // 2
        self.n_mels = cfg.n_mels
        win = _window(window, win_length or n_fft, n_fft)
        basis = None if mel_basis is None else np.ascontiguousarray(mel_basis, np.float32)
        h = C.c_void_p()
        _capi.check(self.ctx.lib.pk_mel_create(self.ctx.handle, C.byref(cfg), _capi.fptr(win),
                                               None if basis is None else _capi.fptr(basis), C.byref(h)))
        self.h = h
        if tid:
            _capi.check(self.ctx.lib.pk_mel_set_transform(h, tid))

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.ctx.lib.pk_mel_destroy(h)
            except Exception:
                pass

    def frames(self, n):
        f = C.c_int32()
        _capi.check(self.ctx.lib.pk_mel_num_frames(self.h, int(n), C.byref(f)))
        return f.value

    def run(self, wavs, what):
        """wavs: list of 1-D arrays -> list of (frames, cols) device tensors."""
        ctx = Context.get(self.ctx.device)
        lens = np.array([int(np.prod(w.shape)) for w in wavs], dtype=np.int32)
        x = torch.cat([ctx.to_device(w).reshape(-1) for w in wavs])
        cols = {0: 2 * self.n_bin, 1: self.n_bin, 2: self.n_mels, 3: 1}[what]
        nf = [self.frames(n) for n in lens]
        out = ctx.empty((sum(nf), cols))
        _capi.check(ctx.lib.pk_mel_run(self.h, dptr(x), lens.ctypes.data_as(C.POINTER(C.c_int32)), len(wavs),
                                       dptr(out), what, 0))
        res, o = [], 0
        for f in nf:
            res.append(out[o:o + f])
            o += f
        return res


class STFT:
    """(B, T) -> real, imag (B, n_bin, frames); audio.py:74-215."""

    def __init__(self, n_fft, hop_length=None, win_length=None, window="hanning", center=True, pad_mode="reflect",
                 transform="dense"):
        if pad_mode != "reflect":
            raise NotImplementedError("only pad_mode='reflect' is implemented")
        win_length = win_length or n_fft
        hop_length = hop_length or int(win_length // 4)
        self.n_fft, self.hop_length, self.n_bin, self.center = n_fft, hop_length, 1 + n_fft // 2, center
        self._mag = _Engine(n_fft, hop_length, win_length, window, center, False, None, 0, transform=transform)
        self._pow = None
        self._args = (n_fft, hop_length, win_length, window, center)
        self.transform = transform

    def _batch(self, x, eng, what):
        x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        outs = eng.run([x[b] for b in range(x.shape[0])], what)
        return torch.stack([o.transpose(0, 1) for o in outs], 0)

    def forward(self, x):
        y = self._batch(x, self._mag, 0)
        return wrap(y[:, :self.n_bin]), wrap(y[:, self.n_bin:])

    __call__ = forward

    def power(self, x):
        if self._pow is None:
            n_fft, hop, win, window, center = self._args
            self._pow = _Engine(n_fft, hop, win, window, center, True, None, 0, transform=self.transform)
        return wrap(self._batch(x, self._pow, 1))

    def magnitude(self, x):
        return wrap(self._batch(x, self._mag, 1))


class _InvEngine:
    """A pk_istft handle: packed (frames, 2*n_bin) re | im rows -> samples, and the Griffin-Lim loop around it."""

    def __init__(self, n_fft, hop_length, win_length, window, center, device=None, transform="dense"):
        tid = _transform_id(transform)
        self.transform = transform
        self.ctx = Context.get(device)
        cfg = _capi.IstftCfg(n_fft, hop_length, 1 if center else 0)
        self.n_fft, self.n_bin = n_fft, 1 + n_fft // 2
        win = _window(window, win_length or n_fft, n_fft)
        h = C.c_void_p()
        _capi.check(self.ctx.lib.pk_istft_create(self.ctx.handle, C.byref(cfg), _capi.fptr(win), C.byref(h)))
        self.h = h
        if tid:
            _capi.check(self.ctx.lib.pk_istft_set_transform(h, tid))

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.ctx.lib.pk_istft_destroy(h)
            except Exception:
                pass

    def samples(self, frames):
        n = C.c_int32()
        _capi.check(self.ctx.lib.pk_istft_num_samples(self.h, int(frames), C.byref(n)))
        return n.value

    def _rows(self, mats, cols, what):
        ctx = Context.get(self.ctx.device)
        mats = [ctx.to_device(m) for m in mats]
        for m in mats:
            if m.dim() != 2 or m.shape[1] != cols:
                raise AssertionError(f"{what}: expected (frames, {cols}) rows, got {tuple(m.shape)}")
        return ctx, torch.cat(mats), np.array([m.shape[0] for m in mats], dtype=np.int32)

    def _out(self, ctx, frames):
        # at least one float: an empty tensor has no address to hand to the engine (which refuses frames < 1 itself)
        return ctx.empty((max(1, sum(self.samples(f) for f in frames if f >= 1)),))

    def _split(self, out, frames):
        res, o = [], 0
        for f in frames:
            n = self.samples(f)
            res.append(out[o:o + n])
            o += n
        return res

    def run(self, specs):
        """specs: list of (frames_b, 2*n_bin) re | im -> list of (T_b,) device tensors."""
        ctx, x, frames = self._rows(specs, 2 * self.n_bin, "ISTFT")
        out = self._out(ctx, frames)
        _capi.check(ctx.lib.pk_istft_run(self.h, dptr(x), frames.ctypes.data_as(C.POINTER(C.c_int32)), len(frames),
                                         dptr(out), 0))
        return self._split(out, frames)

    def griffin_lim(self, stft_engine, mags, n_iter=32, momentum=0.99, seeds=None, angles=None):
        """mags: list of (frames_b, n_bin); angles: None or a list of (frames_b, 2*n_bin) cos | sin; seeds: None or one
        integer per utterance -> list of (T_b,) device tensors."""
        ctx, s, frames = self._rows(mags, self.n_bin, "Griffin-Lim magnitudes")
        a = None
        if angles is not None:
            _, a, fa = self._rows(angles, 2 * self.n_bin, "Griffin-Lim angles")
            if not np.array_equal(fa, frames):
                raise AssertionError("Griffin-Lim: angles and magnitudes differ in their frame counts")
        sd = None
        if seeds is not None:
            sd = np.array([int(v) & (2 ** 64 - 1) for v in seeds], dtype=np.uint64)
            if sd.size != len(frames):
                raise AssertionError("Griffin-Lim: one seed per utterance is needed")
        out = self._out(ctx, frames)
        _capi.check(ctx.lib.pk_gl_run(self.h, stft_engine.h, dptr(s), frames.ctypes.data_as(C.POINTER(C.c_int32)),
                                      len(frames), int(n_iter), float(momentum),
                                      None if sd is None else sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      None if a is None else dptr(a), dptr(out), 0))
        return self._split(out, frames)


class ISTFT:
    """real, imag (B, n_bin, frames) -> (B, T): the inverse of ``STFT`` (librosa's ``istft``, audio.py:86-93)."""

    def __init__(self, n_fft, hop_length=None, win_length=None, window="hanning", center=True, transform="dense"):
        win_length = win_length or n_fft
        hop_length = hop_length or int(win_length // 4)
        self.n_fft, self.hop_length, self.n_bin, self.center = n_fft, hop_length, 1 + n_fft // 2, center
        self._eng = _InvEngine(n_fft, hop_length, win_length, window, center, transform=transform)

    def forward(self, real, imag):
        ctx = Context.get()
        real, imag = ctx.to_device(real), ctx.to_device(imag)
        if real.dim() != 3 or real.shape != imag.shape or real.shape[1] != self.n_bin:
            raise AssertionError(f"ISTFT: expected two (B, {self.n_bin}, frames) tensors, got {tuple(real.shape)} and "
                                 f"{tuple(imag.shape)}")
        rows = torch.cat([real, imag], 1).transpose(1, 2).contiguous()          # (B, frames, re | im)
        return wrap(torch.stack(self._eng.run([rows[b] for b in range(rows.shape[0])]), 0))

    __call__ = forward

    def inverse_batch(self, specs):
        """Ragged: a list of (frames_b, 2*n_bin) re | im rows (``pk_mel_run`` what = 0) -> a list of (T_b,)."""
        return [wrap(o) for o in self._eng.run(list(specs))]


class MelScale:
    """(B, n_freq, frames) -> (B, n_mels, frames); audio.py:218-229 (a plain matmul with the basis)."""

    def __init__(self, sr, n_fft, n_mels, fmin, fmax):
        self.weight = torch.from_numpy(mel_filterbank(sr, n_fft, n_mels, fmin, fmax))
        self._wkn = np.ascontiguousarray(self.weight.numpy().T)          # [n_freq][n_mels]

    def forward(self, spec):
        """``paddle.matmul(self.weight, spectrogram)`` as one engine GEMM over rows = (batch, frame)
        (``pk_op_matmul``); torch only moves data (the NCL <-> rows transposes)."""
        ctx = Context.get()
        spec = ctx.to_device(spec)
        squeeze = spec.dim() == 2
        if squeeze:
            spec = spec[None]
        B, F, T = spec.shape
        assert F == self._wkn.shape[0], "MelScale: spectrogram has the wrong number of frequency bins"
        n_mels = self._wkn.shape[1]
        x = spec.transpose(1, 2).contiguous().reshape(B * T, F)
        y = ctx.empty((B * T, n_mels))
        _capi.check(ctx.lib.pk_op_matmul(ctx.handle, dptr(x), B * T, F, n_mels, _capi.fptr(self._wkn), None, dptr(y)))
        out = y.reshape(B, T, n_mels).transpose(1, 2).contiguous()
        return wrap(out[0] if squeeze else out)

    __call__ = forward


class LogMelFBank:
    """get_feats.py:20-88 on the device: wav -> (num_frames, n_mels) log-mel."""

    def __init__(self, sr=24000, n_fft=2048, hop_length=300, win_length=None, window="hann", n_mels=80,
                 fmin=80, fmax=7600, eps=1e-10, transform="dense"):
        _transform_id(transform)
        self.transform = transform
        self.sr, self.n_fft, self.hop_length = sr, n_fft, hop_length
        self.fmin = 0 if fmin is None else fmin
        self.fmax = sr / 2 if fmax is None else fmax
        self.mel_filter = mel_filterbank(sr, n_fft, n_mels, self.fmin, self.fmax)
        self._args = (n_fft, hop_length, win_length or n_fft, window)
        self._eng = {}

    def _engine(self, base):
        if base not in self._eng:
            n_fft, hop, win, window = self._args
            self._eng[base] = _Engine(n_fft, hop, win, window, True, False, self.mel_filter,
                                      10 if base == "10" else 2, transform=self.transform)
        return self._eng[base]

    def get_log_mel_fbank(self, wav, base="10", sr=None):
        """``sr``: the rate ``wav`` is at, when it is not the extractor's: it is resampled on the engine first."""
        if sr is not None and int(sr) != int(self.sr):
            wav = _resampler(sr, self.sr)(wav)
        return wrap(self._engine(base).run([wav], 2)[0])

    def get_log_mel_fbank_batch(self, wavs, base="10"):
        return [wrap(o) for o in self._engine(base).run(list(wavs), 2)]


def average_by_duration_numpy(x, d):
    """The reference's loop (get_feats.py:205-214; ``Pitch._average_by_duration`` :141-153 is the same plain mean, its
    mask line changes nothing) as one vectorised host expression: the mean of ``x[cum[t-1]:cum[t]]`` per token, 0 for
    a token of 0 frames.  (T,) for 1-D ``x``, (T, C) otherwise."""
    x = np.asarray(x)
    d = np.asarray(d, dtype=np.int64).reshape(-1)
    cum = np.minimum(np.concatenate([[0], np.cumsum(d)]), x.shape[0])
    csum = np.concatenate([np.zeros((1,) + x.shape[1:], np.float64), np.cumsum(x.astype(np.float64), axis=0)], axis=0)
    n = (cum[1:] - cum[:-1]).reshape((-1,) + (1,) * (x.ndim - 1))
    tot = csum[cum[1:]] - csum[cum[:-1]]
    return np.where(n > 0, tot / np.maximum(n, 1), 0.0).astype(x.dtype if x.dtype.kind == "f" else np.float64)


def average_by_duration(x, d):
    """Token averages of a frame-level feature on the engine (``pk_op_average_by_duration``): ``x`` (frames,) or
    (frames, C), ``d`` (T,) integer durations -> device tensor (T,) / (T, C); 0 for a token of 0 frames."""
    ctx = Context.get()
    xt = ctx.to_device(x)
    one_d = xt.dim() == 1
    xt = xt.reshape(xt.shape[0], -1)
    dur = np.ascontiguousarray(np.asarray(d.cpu() if isinstance(d, torch.Tensor) else d).astype(np.int64).reshape(-1))
    out = ctx.empty((dur.size, xt.shape[1]))
    if dur.size:
        _capi.check(ctx.lib.pk_op_average_by_duration(ctx.handle, dptr(xt), xt.shape[0], xt.shape[1],
                                                      dur.ctypes.data_as(C.POINTER(C.c_int64)), dur.size, dptr(out)))
    return wrap(out[:, 0] if one_d else out)


class Energy:
    """get_feats.py:167-220 on the device: per frame ``sqrt(clip(sum_bins |STFT|^2, 1e-10))``, reduced in the kernel that
    reads the frame's spectrum (``pk_mel_run`` what = 3)."""

    def __init__(self, sr=24000, n_fft=2048, hop_length=300, win_length=None, window="hann", center=True,
                 pad_mode="reflect"):
        if pad_mode != "reflect":
            raise NotImplementedError("only pad_mode='reflect' is implemented")
        self.sr, self.n_fft, self.hop_length, self.win_length = sr, n_fft, hop_length, win_length
        self.window, self.center, self.pad_mode = window, center, pad_mode
        self._eng = _Engine(n_fft, hop_length, win_length or n_fft, window, center, False, None, 0)

    def _calculate_energy(self, input):   # noqa: A002  (the reference's argument name)
        return wrap(self._eng.run([input], 3)[0][:, 0])

    def get_energy_batch(self, wavs):
        return [wrap(o[:, 0]) for o in self._eng.run(list(wavs), 3)]

    def get_energy(self, wav, use_token_averaged_energy=True, duration=None):
        """(frames,) energy, or with ``duration`` its token averages (T, 1) like the reference's."""
        energy = self._calculate_energy(wav)
        if use_token_averaged_energy and duration is not None:
            energy = wrap(average_by_duration(energy, duration).reshape(-1, 1))
        return energy

# ---- pitch -----------------------------------------------------------------------------------------------------------
# the engine's envelope (csrc/pk_pitch.h)
PITCH_MAX_TAU, PITCH_MAX_HOP = 960, 16384
PITCH_MAX_CANDIDATES, PITCH_MAX_TRACK_FRAMES, PITCH_TRACK_LDS_FRAMES = 8, 1 << 22, 4096
PITCH_TRACKERS = ("frame", "viterbi")


def pitch_lags(sr, f0min, f0max):
    """(tau_min, tau_max) of DESIGN.md 4.5e: tau_max = ceil(sr / f0min), tau_min = max(2, floor(sr / f0max)); ``ValueError``
    unless 0 < f0min < f0max, sr > 0 and tau_min <= tau_max - 2."""
    if not sr > 0 or not f0min > 0 or not f0max > 0:
        raise ValueError(f"pitch: sr = {sr}, f0min = {f0min}, f0max = {f0max} must be positive")
    if not f0max > f0min:
        raise ValueError(f"pitch: f0max = {f0max} must be above f0min = {f0min}")
    tau_max = int(math.ceil(Fraction(sr) / Fraction(f0min)))
    tau_min = max(2, int(math.floor(Fraction(sr) / Fraction(f0max))))
    if tau_min > tau_max - 2:
        raise ValueError(f"pitch: lags {tau_min} ... {tau_max} (sr = {sr}, f0min = {f0min}, f0max = {f0max}) leave no lag "
                         "with a neighbour on either side: tau_min <= tau_max - 2 is needed")
    return tau_min, tau_max


def _check_pitch_envelope(hop_length, tau_max, win_length):
    if tau_max > PITCH_MAX_TAU:
        raise NotImplementedError(f"pitch: tau_max = ceil(sr / f0min) = {tau_max} lags; the engine's limit is {PITCH_MAX_TAU} "
                                  "(48 kHz at f0min = 50 Hz)")
    if not 1 <= win_length <= 2 * tau_max:
        raise NotImplementedError(f"pitch: win_length = {win_length}; the engine's limit is 1 ... 2 * tau_max = {2 * tau_max}")
    if not 1 <= hop_length <= PITCH_MAX_HOP:
        raise NotImplementedError(f"pitch: hop_length = {hop_length}; the engine's limit is 1 ... {PITCH_MAX_HOP}")


def continuous_f0_batch(f0s, use_log_f0=False, device=None, fill=True):
    """``Pitch._convert_to_continuous_f0`` (get_feats.py:99-119) for a ragged list of f0 tracks from ANY estimator, then the
    natural log of the non-zero values if asked (:136-138): one engine call (``pk_op_continuous_f0``) -> list of (frames,)
    device tensors.  ``fill=False`` leaves the unvoiced frames at zero (the reference's ``use_continuous_f0=False``)."""
    ctx = Context.get(device)
    xs = [ctx.to_device(f).reshape(-1) for f in f0s]
    if not xs:
        return []
    frames = np.array([x.numel() for x in xs], dtype=np.int32)
    if frames.min() < 1:
        raise ValueError("continuous f0: an empty track")
    x = xs[0].contiguous() if len(xs) == 1 else torch.cat(xs)
    out = ctx.empty((int(frames.sum()),))
    _capi.check(ctx.lib.pk_op_continuous_f0(ctx.handle, dptr(x), frames.ctypes.data_as(C.POINTER(C.c_int32)), len(xs),
                                            (1 if use_log_f0 else 0) | (0 if fill else 2), dptr(out)))
    res, o = [], 0
    for n in frames:
        res.append(wrap(out[o:o + n]))
        o += n
    return res


class Pitch:
    """get_feats.py:91-164 on the device, with this project's estimator in place of pyworld's.

    The reference's ``_calculate_f0`` calls DIO + StoneMask (third-party C++); what runs here is NOT that: it is the estimator
    defined in DESIGN.md 4.5e (YIN's difference function, cumulative-mean normalisation, absolute ``threshold`` and
    parabolic refinement; csrc/pitch.hip), which returns f0 in Hz on the same frame grid (``len(wav) // hop_length + 1``
    frames) with its own voicing decisions.  Everything after the estimator is the reference's: continuous f0, the log of the
    non-zero values, token averages.  Results are device tensors, as ``Energy`` returns them.

    ``tracker="frame"`` (the default) decides every frame on its own.  ``tracker="viterbi"`` puts a second decision stage behind
    the same d': up to ``max_candidates`` (1 ... 8) local minima of d' under ``candidate_threshold`` per frame, and the cheapest
    path over them with ``octave_cost`` per octave between consecutive voiced frames, ``unvoiced_cost`` (default: ``threshold``)
    per unvoiced frame and ``switch_cost`` per change of voicing (this project's own design too; checked on
    synthetic signals only).  ``track``, ``_calculate_f0``, ``get_pitch`` and ``get_pitch_batch`` follow the handle's tracker."""

    def __init__(self, sr=24000, hop_length=300, f0min=80, f0max=7600, *, threshold=0.1, win_length=None, device=None,
                 tracker="frame", max_candidates=8, candidate_threshold=0.5, octave_cost=1.0, unvoiced_cost=None,
                 switch_cost=0.05):
        self.sr, self.hop_length, self.f0min, self.f0max = sr, hop_length, f0min, f0max
        if tracker not in PITCH_TRACKERS:
            raise ValueError(f"pitch: tracker = {tracker!r}; one of {PITCH_TRACKERS}")
        if int(max_candidates) != max_candidates or not 1 <= max_candidates <= PITCH_MAX_CANDIDATES:
            raise ValueError(f"pitch: max_candidates = {max_candidates} must be an integer in 1 ... {PITCH_MAX_CANDIDATES}")
        if candidate_threshold != candidate_threshold:
            raise ValueError("pitch: candidate_threshold is not a number")
        costs = dict(octave_cost=octave_cost, switch_cost=switch_cost,
                     unvoiced_cost=threshold if unvoiced_cost is None else unvoiced_cost)
        for name, v in costs.items():
            if not (0 <= v < math.inf):
                raise ValueError(f"pitch: {name} = {v} must be a finite number >= 0")
        self.tracker, self.max_candidates, self.candidate_threshold = tracker, int(max_candidates), float(candidate_threshold)
        self.octave_cost, self.switch_cost, self.unvoiced_cost = (float(costs[k]) for k in ("octave_cost", "switch_cost",
                                                                                            "unvoiced_cost"))
        self.tau_min, self.tau_max = pitch_lags(sr, f0min, f0max)
        if int(sr) != sr or int(hop_length) != hop_length or hop_length < 1:
            raise ValueError(f"pitch: sr = {sr} and hop_length = {hop_length} must be positive integers")
        if not 0 < threshold:
            raise ValueError(f"pitch: threshold = {threshold} must be positive")
        self.threshold = float(threshold)
        self.win_length = 2 * self.tau_max if win_length is None else int(win_length)
        _check_pitch_envelope(int(hop_length), self.tau_max, self.win_length)
        self._device = device
        self.ctx = Context.get(device)
        cfg = _capi.PitchCfg(int(sr), int(hop_length), self.tau_min, self.tau_max, self.win_length, self.threshold)
        h = C.c_void_p()
        _capi.check(self.ctx.lib.pk_pitch_create(self.ctx.handle, C.byref(cfg), C.byref(h)))
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.ctx.lib.pk_pitch_destroy(h)
            except Exception:
                pass

    def frames(self, n):
        return int(n) // int(self.hop_length) + 1

    @property
    def tile_frames(self):
        """Frames per workgroup of the engine's kernel."""
        t = C.c_int32()
        _capi.check(self.ctx.lib.pk_pitch_tile_frames(self.h, C.byref(t)))
        return t.value

    def _run(self, wavs, want_lag=False, want_cmnd=False):
        ctx = Context.get(self._device)
        xs = [ctx.to_device(w).reshape(-1) for w in wavs]
        lens = np.array([x.numel() for x in xs], dtype=np.int32)
        if lens.size == 0 or lens.min() < 1:
            raise ValueError("Pitch: an empty signal")
        x = xs[0].contiguous() if len(xs) == 1 else torch.cat(xs)
        nf = [self.frames(n) for n in lens]
        total = sum(nf)
        f0 = ctx.empty((total,))
        lag = torch.empty((total,), dtype=torch.int32, device=f0.device) if want_lag else None
        cm = ctx.empty((total, self.tau_max + 1)) if want_cmnd else None
        _capi.check(ctx.lib.pk_pitch_run(self.h, dptr(x), lens.ctypes.data_as(C.POINTER(C.c_int32)), len(xs), dptr(f0),
                                         None if lag is None else C.c_void_p(lag.data_ptr()),
                                         None if cm is None else dptr(cm), 0))
        split = lambda t: None if t is None else list(torch.split(t, nf))   # noqa: E731
        return split(f0), split(lag), split(cm)

    def track(self, wavs):
        """Ragged list -> per utterance ``(f0_raw, lag)``: (frames,) float32 Hz (0 for unvoiced) and int32 lags (0), decided by the
        handle's ``tracker``."""
        if self.tracker == "viterbi":
            return self.track_viterbi(wavs)
        f0, lag, _ = self._run(list(wavs), want_lag=True)
        return [(wrap(a), b) for a, b in zip(f0, lag)]

    # ---- Viterbi tracking over candidates
    def set_track_lds_frames(self, n):
        """Tracks of more than ``n`` frames (1 ... 4096, the default) keep the tracker's backpointers in a global workspace
        instead of LDS.  The results do not change."""
        if int(n) != n or not 1 <= n <= PITCH_TRACK_LDS_FRAMES:
            raise ValueError(f"pitch: track_lds_frames = {n} must be an integer in 1 ... {PITCH_TRACK_LDS_FRAMES}")
        _capi.check(self.ctx.lib.pk_pitch_set_option(self.h, b"track_lds_frames", int(n)))

    def _track_cfg(self):
        return _capi.PitchTrackCfg(self.max_candidates, self.candidate_threshold, self.octave_cost, self.unvoiced_cost,
                                   self.switch_cost)

    def _track_outputs(self, ctx, nf, want_cand):
        total, K = sum(nf), self.max_candidates
        f0 = ctx.empty((total,))
        lag = torch.empty((total,), dtype=torch.int32, device=f0.device)
        score = torch.empty((len(nf),), dtype=torch.float64, device=f0.device)
        cl = torch.empty((total, K), dtype=torch.int32, device=f0.device) if want_cand else None
        cc = ctx.empty((total, K)) if want_cand else None
        return f0, lag, score, cl, cc

    def _run_track(self, wavs, want_cand=False):
        """-> per utterance lists (f0, lag, candidate lags, candidate costs) and the (B,) float64 scores: one engine call."""
        ctx = Context.get(self._device)
        xs, lens, x = _pack(ctx, list(wavs), "Pitch")
        nf = [self.frames(n) for n in lens]
        if max(nf) > PITCH_MAX_TRACK_FRAMES:
            raise NotImplementedError(f"pitch: a track of {max(nf)} frames; the tracker's limit is {PITCH_MAX_TRACK_FRAMES}")
        f0, lag, score, cl, cc = self._track_outputs(ctx, nf, want_cand)
        cfg = self._track_cfg()
        _capi.check(ctx.lib.pk_pitch_track_run(self.h, dptr(x), _i32p(lens), len(xs), C.byref(cfg), dptr(f0), _vptr(lag),
                                               _vptr(score), _vptr(cl), _vptr(cc), 0))
        split = lambda t: None if t is None else list(torch.split(t, nf))   # noqa: E731
        return split(f0), split(lag), split(cl), split(cc), score

    def candidates(self, wavs):
        """Ragged list -> per utterance ``(lags, costs)``: (frames, max_candidates) int32 and float32, a frame's candidates by
        ascending lag, empty slots with lag 0 and cost +inf."""
        _, _, cl, cc, _ = self._run_track(wavs, want_cand=True)
        return [(a, wrap(b)) for a, b in zip(cl, cc)]

    def track_viterbi(self, wavs, return_score=False):
        """Ragged list -> per utterance ``(f0_raw, lag)`` of the Viterbi path over the frames' candidates, whatever the
        handle's ``tracker`` is; with ``return_score`` ``(f0_raw, lag, score)``, the path's cost as a float."""
        f0, lag, _, _, score = self._run_track(wavs)
        if not return_score:
            return [(wrap(a), b) for a, b in zip(f0, lag)]
        return [(wrap(a), b, float(c)) for a, b, c in zip(f0, lag, score.cpu())]

    def track_from_cmnd(self, rows):
        """A list of (frames, tau_max + 1) d' arrays (``cmnd``'s layout) -> per track a dict of ``f0``, ``lag``, ``score``
        (float), ``cand_lag`` and ``cand_cost``: the tracker on rows of the caller."""
        ctx = Context.get(self._device)
        rs = [ctx.to_device(r) for r in rows]
        if not rs:
            return []
        for r in rs:
            if r.dim() != 2 or r.shape[1] != self.tau_max + 1:
                raise ValueError(f"pitch: d' rows of shape {tuple(r.shape)}; (frames, tau_max + 1 = {self.tau_max + 1}) is needed")
        nf = [int(r.shape[0]) for r in rs]
        if min(nf) < 1:
            raise ValueError("pitch: an empty track")
        if max(nf) > PITCH_MAX_TRACK_FRAMES:
            raise NotImplementedError(f"pitch: a track of {max(nf)} frames; the tracker's limit is {PITCH_MAX_TRACK_FRAMES}")
        x = rs[0].contiguous() if len(rs) == 1 else torch.cat(rs)
        f0, lag, score, cl, cc = self._track_outputs(ctx, nf, True)
        cfg = self._track_cfg()
        _capi.check(ctx.lib.pk_pitch_track_from_cmnd(self.h, dptr(x), _i32p(np.array(nf, dtype=np.int32)), len(rs), C.byref(cfg),
                                                     dptr(f0), _vptr(lag), _vptr(score), _vptr(cl), _vptr(cc), 0))
        sc = score.cpu()
        return [dict(f0=wrap(a), lag=b, score=float(c), cand_lag=d, cand_cost=wrap(e))
                for a, b, c, d, e in zip(torch.split(f0, nf), torch.split(lag, nf), sc, torch.split(cl, nf), torch.split(cc, nf))]

    def cmnd(self, wav):
        """(frames, tau_max + 1): the cumulative-mean-normalised difference d'(0 ... tau_max) of every frame."""
        return wrap(self._run([wav], want_cmnd=True)[2][0])

    def _convert_to_continuous_f0(self, f0):
        return continuous_f0_batch([f0], False, self._device)[0]

    def _calculate_f0(self, input, use_continuous_f0=True, use_log_f0=True):   # noqa: A002  (the reference's argument name)
        return self.get_pitch_batch([input], None, use_continuous_f0, use_log_f0)[0]

    def _average_by_duration(self, input, d):   # noqa: A002
        return wrap(average_by_duration(Context.get(self._device).to_device(input).reshape(-1), d).reshape(-1, 1))

    def get_pitch(self, wav, use_continuous_f0=True, use_log_f0=True, use_token_averaged_f0=True, duration=None):
        """(frames,) f0, or with ``duration`` its token averages (T, 1) like the reference's."""
        f0 = self._calculate_f0(wav, use_continuous_f0, use_log_f0)
        if use_token_averaged_f0 and duration is not None:
            f0 = self._average_by_duration(f0, duration)
        return f0

    def get_pitch_batch(self, wavs, durations=None, use_continuous_f0=True, use_log_f0=True, use_token_averaged_f0=True,
                        tracker=None):
        """``get_pitch`` for a ragged list: one engine call for the estimator and one for the continuous / log step.
        ``tracker`` overrides the handle's for this call."""
        wavs = list(wavs)
        tracker = self.tracker if tracker is None else tracker
        if tracker not in PITCH_TRACKERS:
            raise ValueError(f"pitch: tracker = {tracker!r}; one of {PITCH_TRACKERS}")
        f0 = self._run_track(wavs)[0] if tracker == "viterbi" else self._run(wavs)[0]
        if use_continuous_f0 or use_log_f0:
            f0 = continuous_f0_batch(f0, use_log_f0, self._device, fill=use_continuous_f0)
        f0 = [wrap(f) for f in f0]
        if use_token_averaged_f0 and durations is not None:
            f0 = [self._average_by_duration(f, d) for f, d in zip(f0, durations)]
        return f0


# ---- silence trimming ------------------------------------------------------------------------------------------------
# DESIGN.md 4.5f.  The frame test of trim / split is librosa 0.8's (librosa is not a dependency: the definition in DESIGN.md is
# the contract); everything after the voice detector in trim_long_silences is the reference's; the energy detector in front of
# it is this project's own, NOT webrtcvad.  The engine's envelope (csrc/pk_trim.h):
TRIM_MAX_FRAME, TRIM_MAX_AVG, TRIM_MAX_SILENCE = 16384, 64, 64
_TRIM_HANDLES = {}


class _TrimEngine:
    """One ``pk_trim`` handle (workspaces only) per device."""

    def __init__(self, device=None):
        self.ctx = Context.get(device)
        h = C.c_void_p()
        _capi.check(self.ctx.lib.pk_trim_create(self.ctx.handle, C.byref(h)))
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.ctx.lib.pk_trim_destroy(h)
            except Exception:
                pass


def _trim_engine(device=None):
    ctx = Context.get(device)
    key = str(ctx.device)
    if key not in _TRIM_HANDLES:
        _TRIM_HANDLES[key] = _TrimEngine(device)
    return _TRIM_HANDLES[key]


def _pack(ctx, wavs, what):
    """A ragged list -> (device tensors, lens int32, the packed buffer)."""
    xs = [ctx.to_device(w).reshape(-1) for w in wavs]
    lens = np.array([x.numel() for x in xs], dtype=np.int32)
    if lens.size == 0 or lens.min() < 1:
        raise ValueError(f"{what}: an empty signal")
    return xs, lens, xs[0].contiguous() if len(xs) == 1 else torch.cat(xs)


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _vptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _check_frame_envelope(frame_length, hop_length):
    if int(frame_length) != frame_length or int(hop_length) != hop_length or frame_length < 1 or hop_length < 1:
        raise ValueError(f"frame_length = {frame_length} and hop_length = {hop_length} must be positive integers")
    if frame_length > TRIM_MAX_FRAME:
        raise NotImplementedError(f"frame_length = {frame_length}; the engine's limit is {TRIM_MAX_FRAME}")
    if hop_length > frame_length:
        raise NotImplementedError(f"hop_length = {hop_length}; the engine's limit is 1 ... frame_length = {frame_length}")


def _pad_mode(center, pad_mode):
    if not center:
        return 0
    if pad_mode not in ("reflect", "constant"):
        raise ValueError(f"pad_mode must be 'reflect' or 'constant', got {pad_mode!r}")
    return _capi.PK_TRIM_PAD[pad_mode]


def trim_num_frames(n, frame_length, hop_length, center=True):
    """1 + (n + 2 (frame_length // 2) - frame_length) // hop_length when centred, 1 + (n - frame_length) // hop_length (0 for
    n < frame_length) when not."""
    padded = int(n) + (2 * (int(frame_length) // 2) if center else 0)
    return 0 if padded < frame_length else 1 + (padded - int(frame_length)) // int(hop_length)


def trim_tile_frames(frame_length=2048, hop_length=512):
    """Frames per workgroup of the engine's power kernel."""
    _check_frame_envelope(frame_length, hop_length)
    t = C.c_int32()
    _capi.check(_capi.lib().pk_trim_tile_frames(int(frame_length), int(hop_length), C.byref(t)))
    return t.value


def _trim_run(wavs, frame_length, hop_length, center, pad_mode, top_db=None, rms=False, device=None):
    """One engine call -> per utterance P (or its root), and with ``top_db`` the flags (bool) and a (B, 2) int32 device tensor
    of (start, end); None where not asked for."""
    _check_frame_envelope(frame_length, hop_length)
    mode = _pad_mode(center, pad_mode)
    sizes = [int(np.prod(w.shape)) if hasattr(w, "shape") else len(w) for w in wavs]
    if not sizes or min(sizes) < 1:
        raise ValueError("trim: an empty signal")
    if mode == 1 and min(sizes) <= frame_length // 2:
        raise ValueError(f"reflect padding needs more than frame_length // 2 = {frame_length // 2} samples, got {min(sizes)}")
    eng = _trim_engine(device)
    ctx = eng.ctx
    xs, lens, x = _pack(ctx, wavs, "trim")
    nf = [trim_num_frames(n, frame_length, hop_length, bool(center)) for n in lens]
    power = ctx.empty((sum(nf),))
    if sum(nf) == 0:                                   # center=False and no signal as long as a frame
        return ([wrap(ctx.empty((0,))) for _ in xs], [ctx.empty((0,), torch.bool) for _ in xs],
                torch.zeros((len(xs), 2), dtype=torch.int32, device=power.device))
    flags = bounds = None
    factor = 1.0
    if top_db is not None:
        factor = 10.0 ** (-float(top_db) / 10.0)
        flags = torch.empty((sum(nf),), dtype=torch.bool, device=power.device)    # (the kernel writes bytes 0 / 1)
        bounds = torch.empty((len(xs), 2), dtype=torch.int32, device=power.device)
    _capi.check(ctx.lib.pk_trim_run(eng.h, dptr(x), _i32p(lens), len(xs), int(frame_length), int(hop_length), mode, factor,
                                    1 if rms else 0, _vptr(power), _vptr(flags), _vptr(bounds)))
    P = [wrap(p) for p in torch.split(power, nf)]
    F = None if flags is None else list(torch.split(flags, nf))
    return P, F, bounds


def frame_power(wavs, frame_length=2048, hop_length=512, center=True, pad_mode="reflect", device=None):
    """A ragged list of signals -> a list of (frames,) device tensors: the mean of x^2 over every frame.
    ``center=False``: no padding, frames at multiples of the hop.  One engine call."""
    return _trim_run(list(wavs), frame_length, hop_length, center, pad_mode, device=device)[0]


def rms(wavs, frame_length=2048, hop_length=512, center=True, pad_mode="reflect", device=None):
    """The square root of ``frame_power`` (``librosa.feature.rms`` per utterance, without the leading axis)."""
    return _trim_run(list(wavs), frame_length, hop_length, center, pad_mode, rms=True, device=device)[0]


def nonsilent_frames_batch(wavs, top_db=60, frame_length=2048, hop_length=512, pad_mode="reflect", device=None):
    """A list of (frames,) bool device tensors: frame i is non-silent iff 10 log10(max(1e-10, P[i])) - 10 log10(max(1e-10,
    max P)) > -top_db (librosa 0.8's ``_signal_to_frame_nonsilent`` with ``ref=np.max``)."""
    return _trim_run(list(wavs), frame_length, hop_length, True, pad_mode, top_db=top_db, device=device)[1]


def trim_batch(wavs, top_db=60, frame_length=2048, hop_length=512, pad_mode="reflect", device=None):
    """``trim`` for a ragged list in one engine call -> (list of slices ``y[start:end]``, (B, 2) int64 numpy array).  The
    slices are views of what was passed in (numpy stays numpy, a tensor stays a tensor); the only read-back is the B pairs."""
    wavs = list(wavs)
    index = _trim_run(wavs, frame_length, hop_length, True, pad_mode, top_db=top_db, device=device)[2].cpu().numpy().astype(np.int64)
    wavs = [w if isinstance(w, (np.ndarray, torch.Tensor)) else np.asarray(w) for w in wavs]
    return [w.reshape(-1)[a:b] for w, (a, b) in zip(wavs, index)], index


def trim(y, top_db=60, frame_length=2048, hop_length=512, pad_mode="reflect", device=None):
    """``librosa.effects.trim`` for a 1-D signal: ``(y[start:end], np.array([start, end]))`` with start = the first non-silent
    frame * hop, end = min(len(y), (the last one + 1) * hop), (0, 0) without one.  The slice is a view."""
    out, index = trim_batch([y], top_db, frame_length, hop_length, pad_mode, device)
    return out[0], index[0]


def split(y, top_db=60, frame_length=2048, hop_length=512, pad_mode="reflect", device=None):
    """``librosa.effects.split``: the runs of non-silent frames as an (n, 2) int64 array of sample intervals, the last end
    clipped to len(y).  The flags come from the device, the runs are found on the host."""
    flags = nonsilent_frames_batch([y], top_db, frame_length, hop_length, pad_mode, device)[0].cpu().numpy()
    n = int(np.asarray(y.shape).prod()) if hasattr(y, "shape") else len(y)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], flags.astype(np.int8), [0]])))
    return np.minimum(edges.reshape(-1, 2).astype(np.int64) * int(hop_length), n)


def peak_normalize_batch(wavs, device=None):
    """y / max|y| per utterance (``librosa.util.normalize`` of a 1-D signal with its defaults), one rounding per sample; an
    utterance whose max|y| is below float32's smallest normal number comes back unchanged.  A list of device tensors."""
    eng = _trim_engine(device)
    ctx = eng.ctx
    xs, lens, x = _pack(ctx, list(wavs), "peak_normalize")
    out = ctx.empty((int(lens.sum()),))
    _capi.check(ctx.lib.pk_peak_normalize(eng.h, dptr(x), _i32p(lens), len(xs), dptr(out)))
    return [wrap(o) for o in torch.split(out, [int(n) for n in lens])]


def peak_normalize(y, device=None):
    return peak_normalize_batch([y], device)[0]


# ---------------------------------------------------------------------- recursive filters and loudness
# csrc/pk_iir.h: cascades of biquads in float64, cut into chunks of 256 samples and stitched by a carry over the chunks; the
# same bits for an utterance alone, in any batch and at any position.  The engine's envelope:
IIR_MAX_SECTIONS, IIR_CHUNK = 8, 256
LOUDNESS_SR_MIN, LOUDNESS_SR_MAX = 8000, 192000
_IIR_HANDLES = {}


class _IIREngine:
    """One ``pk_iir`` handle: the sections and their chunk transition matrix on one device."""

    def __init__(self, sos, device=None):
        self.ctx = Context.get(device)
        self.sos = sos
        h = C.c_void_p()
        _capi.check(self.ctx.lib.pk_iir_create(self.ctx.handle, sos.ctypes.data_as(C.POINTER(C.c_double)), int(sos.shape[0]),
                                               C.byref(h)))
        self.h = h

    def transition(self):
        """The (2 S, 2 S) float64 transition matrix of one chunk, as the device computed it."""
        n = 2 * int(self.sos.shape[0])
        P = np.empty((n, n), dtype=np.float64)
        _capi.check(self.ctx.lib.pk_iir_transition(self.h, P.ctypes.data_as(C.POINTER(C.c_double))))
        return P

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.ctx.lib.pk_iir_destroy(h)
            except Exception:
                pass


def _check_sos(sos):
    """scipy's (S, 6) rows as a contiguous float64 array; the refusals of ``pk_iir_create``, raised before a device is needed."""
    sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64))
    if sos.ndim != 2 or sos.shape[1] != 6 or sos.shape[0] < 1:
        raise ValueError(f"sos must have shape (n_sections >= 1, 6), got {sos.shape}")
    if sos.shape[0] > IIR_MAX_SECTIONS:
        raise NotImplementedError(f"{sos.shape[0]} sections; the engine's limit is {IIR_MAX_SECTIONS}")
    if not np.isfinite(sos).all():
        raise ValueError("sos has a coefficient that is not finite")
    if (sos[:, 3] != 1.0).any():
        raise ValueError("every section must be normalised to a0 = 1 (as scipy.signal.sosfilt requires)")
    return sos


def _iir_engine(sos, device=None):
    sos = _check_sos(sos)
    ctx = Context.get(device)
    key = (str(ctx.device), sos.tobytes())
    if key not in _IIR_HANDLES:
        _IIR_HANDLES[key] = _IIREngine(sos, device)
    return _IIR_HANDLES[key]


def _pack_ragged(ctx, wavs, what):
    """A list of 1-D signals, empty ones allowed -> (lens int32, the packed float32 device buffer)."""
    wavs = list(wavs)
    if not wavs:
        raise ValueError(f"{what}: no signal given")
    for b, w in enumerate(wavs):
        if not hasattr(w, "shape") or len(w.shape) != 1:
            raise ValueError(f"{what}: signal {b} is not 1-D" + (f" (shape {tuple(w.shape)})" if hasattr(w, "shape") else ""))
    xs = [ctx.to_device(w).reshape(-1) for w in wavs]
    lens = np.array([x.numel() for x in xs], dtype=np.int32)
    x = xs[0].contiguous() if len(xs) == 1 else torch.cat(xs)
    if x.numel() == 0:
        x = ctx.empty((1,))                                 # a pointer to pass; nothing of it is read
    return lens, x


def sosfilt_batch(sos, wavs, device=None):
    """``scipy.signal.sosfilt(sos, x)`` for a ragged list of float32 signals in one engine call: float64 inside, zero initial
    state, one float32 rounding per sample.  A list of device tensors.  At most 8 sections (``NotImplementedError`` beyond)."""
    eng = _iir_engine(sos, device)
    ctx = eng.ctx
    lens, x = _pack_ragged(ctx, wavs, "sosfilt")
    out = ctx.empty((max(int(lens.sum()), 1),))
    _capi.check(ctx.lib.pk_iir_run(eng.h, dptr(x), _i32p(lens), len(lens), dptr(out)))
    return [wrap(o) for o in torch.split(out[:int(lens.sum())], [int(n) for n in lens])]


def sosfilt(sos, x, device=None):
    return sosfilt_batch(sos, [x], device)[0]


def _lfilter_sos(b, a):
    b, a = [float(v) for v in np.asarray(b, dtype=np.float64).reshape(-1)], [float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]
    if not b or not a:
        raise ValueError("lfilter: b and a need at least one coefficient each")
    if len(b) > 3 or len(a) > 3:
        raise NotImplementedError(f"lfilter takes up to three coefficients each (got {len(b)} and {len(a)}); factor a longer "
                                  "filter into second-order sections (scipy.signal.tf2sos) and call sosfilt")
    if a[0] == 0.0 or not all(math.isfinite(v) for v in b + a):
        raise ValueError("lfilter: a[0] must not be 0 and every coefficient must be finite")
    b, a = b + [0.0] * (3 - len(b)), a + [0.0] * (3 - len(a))
    return np.array([[b[0] / a[0], b[1] / a[0], b[2] / a[0], 1.0, a[1] / a[0], a[2] / a[0]]], dtype=np.float64)


def lfilter(b, a, x, device=None):
    """``scipy.signal.lfilter`` for ``len(b), len(a) <= 3``: one section, normalised by a[0] on the host."""
    return sosfilt(_lfilter_sos(b, a), x, device)


def lfilter_batch(b, a, wavs, device=None):
    return sosfilt_batch(_lfilter_sos(b, a), wavs, device)


def _check_coef(coef):
    coef = float(coef)
    if not math.isfinite(coef):
        raise ValueError(f"coef = {coef} must be finite")
    return coef


def preemphasis_batch(wavs, coef=0.97, device=None):
    """y[n] = x[n] - coef x[n - 1] (``librosa.effects.preemphasis`` with a zero initial state)."""
    return sosfilt_batch([[1.0, -_check_coef(coef), 0.0, 1.0, 0.0, 0.0]], wavs, device)


def preemphasis(x, coef=0.97, device=None):
    return preemphasis_batch([x], coef, device)[0]


def deemphasis_batch(wavs, coef=0.97, device=None):
    """y[n] = x[n] + coef y[n - 1], the inverse of ``preemphasis``."""
    return sosfilt_batch([[1.0, 0.0, 0.0, 1.0, -_check_coef(coef), 0.0]], wavs, device)


def deemphasis(x, coef=0.97, device=None):
    return deemphasis_batch([x], coef, device)[0]


def _check_loudness_sr(sr):
    if int(sr) != sr or sr < 1:
        raise ValueError(f"sr = {sr} must be a positive integer")
    sr = int(sr)
    if sr % 10 != 0 or not LOUDNESS_SR_MIN <= sr <= LOUDNESS_SR_MAX:
        raise NotImplementedError(f"sr = {sr}: loudness blocks lie on a 100 ms sample grid, which takes a multiple of 10 Hz in "
                                  f"{LOUDNESS_SR_MIN} ... {LOUDNESS_SR_MAX}; resample first")
    return sr


def k_weighting(sr):
    """The K-weighting of ITU-R BS.1770 at rate ``sr`` as a (2, 6) float64 sos array (the shelf, then the high-pass), by the
    formulas libebur128 uses; at 48 000 Hz they reproduce the Recommendation's table.  Host arithmetic in Python floats."""
    sr = _check_loudness_sr(sr)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, hp], dtype=np.float64)


def _loudness_run(wavs, sr, device=None):
    """One engine call -> (ctx, lens, the packed signal, dict of host arrays per utterance: ``mean_power``, ``rel`` (float64),
    ``peak`` (float32), ``gated``, ``gated_abs``, ``blocks`` (int32), ``lufs`` (float64, -inf where no block is kept))."""
    sr = _check_loudness_sr(sr)
    eng = _iir_engine(k_weighting(sr), device)
    ctx = eng.ctx
    lens, x = _pack_ragged(ctx, wavs, "loudness")
    B = len(lens)
    mean, rel = ctx.empty((B,), torch.float64), ctx.empty((B,), torch.float64)
    peak, counts = ctx.empty((B,)), ctx.empty((B * 3,), torch.int32)
    _capi.check(ctx.lib.pk_loudness_run(eng.h, dptr(x), _i32p(lens), B, sr, dptr(mean), dptr(rel), dptr(peak), dptr(counts)))
    host = torch.cat([t.view(torch.uint8) for t in (mean, rel, peak, counts)]).cpu().numpy()     # the one read
    mean_h, rel_h = host[:8 * B].view(np.float64), host[8 * B:16 * B].view(np.float64)
    peak_h, cnt_h = host[16 * B:20 * B].view(np.float32), host[20 * B:].view(np.int32).reshape(B, 3)
    with np.errstate(divide="ignore"):
        lufs = np.where(cnt_h[:, 0] > 0, -0.691 + 10.0 * np.log10(np.where(cnt_h[:, 0] > 0, mean_h, 1.0)), -np.inf)
    return ctx, lens, x, dict(mean_power=mean_h.copy(), rel=rel_h.copy(), peak=peak_h.copy(), gated=cnt_h[:, 0].copy(),
                              gated_abs=cnt_h[:, 1].copy(), blocks=cnt_h[:, 2].copy(), lufs=lufs)


def normalize_loudness_batch(wavs, sr, target_lufs=-23.0, max_peak=None, return_gains=False, device=None):
    """Every utterance scaled to ``target_lufs`` of gated BS.1770 loudness (``metrics.loudness_batch``; this project's own
    restatement for mono, blocks on a 100 ms sample grid): g = 10^((target - LUFS) / 20) in float64 on the host, capped at
    ``max_peak / peak`` when ``max_peak`` is given (and then stepped down in float32 until the rounded peak sample does not
    exceed it), rounded to float32 and applied on the engine with one rounding per sample.  An utterance whose loudness is
    -inf (shorter than 400 ms, or nothing above -70 LUFS) comes back unchanged with gain 1.  A list of device tensors;
    ``return_gains``: also the float32 gains."""
    target = float(target_lufs)
    if not math.isfinite(target):
        raise ValueError(f"target_lufs = {target_lufs} must be finite")
    if max_peak is not None and not (math.isfinite(float(max_peak)) and float(max_peak) > 0.0):
        raise ValueError(f"max_peak = {max_peak} must be a positive finite number")
    ctx, lens, x, m = _loudness_run(wavs, sr, device)
    gains = np.ones(len(lens), dtype=np.float32)
    for b, (lufs, peak) in enumerate(zip(m["lufs"], m["peak"])):
        if not math.isfinite(lufs):
            continue
        g = 10.0 ** ((target - float(lufs)) / 20.0)
        if max_peak is not None and peak > 0:
            g = min(g, float(max_peak) / float(peak))
        g32 = np.float32(g)
        if max_peak is not None:
            while g32 > 0 and float(np.float32(peak) * g32) > float(max_peak):      # the device's product, rounded the same way
                g32 = np.nextafter(g32, np.float32(0))
        gains[b] = g32
    out = ctx.empty((max(int(lens.sum()), 1),))
    _capi.check(ctx.lib.pk_gain_run(ctx.handle, dptr(x), _i32p(lens), len(lens), gains.ctypes.data_as(C.POINTER(C.c_float)),
                                    dptr(out)))
    res = [wrap(o) for o in torch.split(out[:int(lens.sum())], [int(n) for n in lens])]
    return (res, gains) if return_gains else res


def normalize_loudness(y, sr, target_lufs=-23.0, max_peak=None, return_gains=False, device=None):
    out = normalize_loudness_batch([y], sr, target_lufs, max_peak, return_gains, device)
    return (out[0][0], out[1][0]) if return_gains else out[0]


def _check_vad_envelope(window, width, silence):
    if window < 1:
        raise ValueError(f"vad: vad_window_length * sampling_rate // 1000 = {window} samples; a window needs at least one")
    if window > TRIM_MAX_FRAME:
        raise NotImplementedError(f"vad: a window of {window} samples; the engine's limit is {TRIM_MAX_FRAME}")
    if int(width) != width or width < 1 or int(silence) != silence or silence < 0:
        raise ValueError(f"vad: vad_moving_average_width = {width} must be a positive integer, vad_max_silence_length = "
                         f"{silence} a non-negative one")
    if width > TRIM_MAX_AVG:
        raise NotImplementedError(f"vad: vad_moving_average_width = {width}; the engine's limit is {TRIM_MAX_AVG}")
    if silence > TRIM_MAX_SILENCE:
        raise NotImplementedError(f"vad: vad_max_silence_length = {silence}; the engine's limit is {TRIM_MAX_SILENCE}")


def _vad_run(wavs, vad_window_length, vad_moving_average_width, vad_max_silence_length, sampling_rate, voice_flags=None,
             vad_top_db=40, vad_floor_dBFS=-50, device=None, want_detector=False):
    """-> (list of trimmed device tensors, kept windows per utterance, and with ``want_detector`` the window powers and the
    voice flags the engine used, per utterance)."""
    w = int(vad_window_length * sampling_rate) // 1000
    _check_vad_envelope(w, vad_moving_average_width, vad_max_silence_length)
    eng = _trim_engine(device)
    ctx = eng.ctx
    xs, lens, x = _pack(ctx, wavs, "trim_long_silences")
    B = len(xs)
    nw = [int(n) // w for n in lens]
    total = sum(nw)
    empty = lambda: wrap(ctx.empty((0,)))   # noqa: E731
    if total == 0:
        return ([empty() for _ in xs], np.zeros(B, np.int32), [ctx.empty((0,)) for _ in xs],
                [torch.empty((0,), dtype=torch.bool, device=ctx.device) for _ in xs])
    given = None
    if voice_flags is not None:
        voice_flags = list(voice_flags)
        if len(voice_flags) != B:
            raise ValueError(f"trim_long_silences: {len(voice_flags)} flag arrays for {B} signals")
        fl = [ctx.to_device(np.asarray(f.cpu() if isinstance(f, torch.Tensor) else f).astype(bool).reshape(-1), torch.uint8)
              for f in voice_flags]
        for f, n in zip(fl, nw):
            if f.numel() != n:
                raise ValueError(f"trim_long_silences: {f.numel()} voice flags for a signal of {n} windows of {w} samples")
        given = torch.cat(fl)
    power = ctx.empty((total,)) if (want_detector and given is None) else None
    flags = torch.empty((total,), dtype=torch.bool, device=x.device) if want_detector else None   # (bytes 0 / 1)
    pos = torch.empty((total,), dtype=torch.int32, device=x.device)
    kept = np.zeros(B, dtype=np.int32)
    _capi.check(ctx.lib.pk_vad_mask(eng.h, dptr(x), _i32p(lens), B, w, int(vad_moving_average_width), int(vad_max_silence_length),
                                    _vptr(given), 10.0 ** (-float(vad_top_db) / 10.0), 10.0 ** (float(vad_floor_dBFS) / 10.0),
                                    _vptr(power), _vptr(flags), _vptr(pos), _i32p(kept)))
    sizes = [int(k) * w for k in kept]
    out = ctx.empty((sum(sizes),))
    if sum(sizes):
        _capi.check(ctx.lib.pk_vad_gather(eng.h, dptr(x), _i32p(lens), B, w, _vptr(pos), _i32p(kept), dptr(out)))
    res = [wrap(o) for o in torch.split(out, sizes)]
    if not want_detector:
        return res, kept, None, None
    return res, kept, None if power is None else list(torch.split(power, nw)), list(torch.split(flags, nw))


def trim_long_silences_batch(wavs, vad_window_length, vad_moving_average_width, vad_max_silence_length, sampling_rate, *,
                             voice_flags=None, vad_top_db=40, vad_floor_dBFS=-50, device=None):
    """``trim_long_silences`` (examples/ge2e/audio_processor.py:53-107) for a ragged list -> a list of device tensors.

    Windows of ``vad_window_length * sampling_rate // 1000`` samples (the tail is dropped), one voice flag per window, the
    moving average of the flags rounded half to even, a dilation with ``ones(vad_max_silence_length + 1)``, and the samples of
    the kept windows in order.  With ``voice_flags`` (one array per signal, from webrtcvad or anything else) everything runs
    on the engine and is the reference's, exactly.  Without them the flags come from this project's energy detector, which is
    NOT webrtcvad: window k is voiced iff its power exceeds both ``vad_top_db`` below the loudest window and
    ``vad_floor_dBFS``.  The two defaults are design choices that nobody has compared with webrtcvad on speech, and an energy
    detector flags loud noise as voice.  Two engine calls; the host reads the kept counts in between to size the result."""
    return _vad_run(list(wavs), vad_window_length, vad_moving_average_width, vad_max_silence_length, sampling_rate,
                    voice_flags, vad_top_db, vad_floor_dBFS, device)[0]


def energy_voice_flags_batch(wavs, vad_window_length, sampling_rate, vad_top_db=40, vad_floor_dBFS=-50, device=None):
    """What the energy detector (NOT webrtcvad) sees and decides: per signal ``(Q, flags)``, the power of every window
    (float32) and its voice flag (bool), on the device."""
    _, _, Q, flags = _vad_run(list(wavs), vad_window_length, 1, 0, sampling_rate, None, vad_top_db, vad_floor_dBFS, device,
                              want_detector=True)
    return [(wrap(q), f) for q, f in zip(Q, flags)]


def trim_long_silences(wav, vad_window_length, vad_moving_average_width, vad_max_silence_length, sampling_rate, *,
                       voice_flags=None, vad_top_db=40, vad_floor_dBFS=-50, device=None):
    """One signal through ``trim_long_silences_batch``."""
    return trim_long_silences_batch([wav], vad_window_length, vad_moving_average_width, vad_max_silence_length, sampling_rate,
                                    voice_flags=None if voice_flags is None else [voice_flags], vad_top_db=vad_top_db,
                                    vad_floor_dBFS=vad_floor_dBFS, device=device)[0]


# ---- resampling ------------------------------------------------------------------------------------------------------
# name -> (zeros, rolloff, beta): the number of zero crossings kept on each side (at the lower of the two rates), the cutoff as
# a fraction of the lower Nyquist frequency, the Kaiser window's beta.  DESIGN.md 4.5d.
RESAMPLE_FILTERS = {
    "kaiser_best": (64, 0.9475937167399596, 14.769656459379492),
    "kaiser_fast": (16, 0.85, 8.555504641634386),
}
# the engine's envelope (csrc/pk_resample.h)
RESAMPLE_MAX_RATIO, RESAMPLE_MAX_TAPS, RESAMPLE_MAX_TABLE = 4096, 8192, 4 << 20


def _filter_params(res_type, zeros, rolloff, beta):
    if res_type not in RESAMPLE_FILTERS:
        raise ValueError(f"resample: unknown res_type {res_type!r} (one of {sorted(RESAMPLE_FILTERS)})")
    z, r, b = RESAMPLE_FILTERS[res_type]
    zeros, rolloff, beta = (z if zeros is None else zeros, r if rolloff is None else float(rolloff),
                            b if beta is None else float(beta))
    if not zeros > 0 or not 0 < rolloff <= 1 or not beta >= 0:
        raise ValueError(f"resample: zeros = {zeros}, rolloff = {rolloff}, beta = {beta}: need zeros > 0, 0 < rolloff <= 1, "
                         "beta >= 0")
    return zeros, rolloff, beta


def resample_ratio(orig_sr, target_sr):
    """(up, down) = target_sr / orig_sr in lowest terms."""
    if int(orig_sr) != orig_sr or int(target_sr) != target_sr or orig_sr <= 0 or target_sr <= 0:
        raise ValueError(f"resample: sampling rates must be positive integers, got {orig_sr} and {target_sr}")
    fr = Fraction(int(target_sr), int(orig_sr))
    return fr.numerator, fr.denominator


def resample_taps(up, down, zeros):
    """T: taps per phase.  |s tau| < zeros with s = min(1, up / down) admits the input offsets -H ... H - 1 around an output's
    input base, H = ceil(zeros / s)."""
    return 2 * int(math.ceil(zeros * max(up, down) / up))


def _check_resample_envelope(up, down, taps):
    if not (1 <= up <= RESAMPLE_MAX_RATIO and 1 <= down <= RESAMPLE_MAX_RATIO):
        raise NotImplementedError(f"resample: the ratio {up} / {down} in lowest terms is outside the engine's envelope: both "
                                  f"terms must be in 1 ... {RESAMPLE_MAX_RATIO}")
    if taps > RESAMPLE_MAX_TAPS:
        raise NotImplementedError(f"resample: {taps} taps per phase; the engine's limit is {RESAMPLE_MAX_TAPS}")
    if up * taps > RESAMPLE_MAX_TABLE:
        raise NotImplementedError(f"resample: a table of up * taps = {up * taps} coefficients; the engine's limit is "
                                  f"{RESAMPLE_MAX_TABLE}")


def resample_filter(up, down, res_type="kaiser_best", zeros=None, rolloff=None, beta=None):
    """The phase table of DESIGN.md 4.5d, (up, T) float64, numpy only.

    With s = min(1, up / down):  g(tau) = s rolloff sinc(rolloff s tau) K(s tau / zeros) for |s tau| < zeros, else 0;
    K(u) = I0(beta sqrt(1 - u^2)) / I0(beta).  Row p, tap k is g(H - 1 - k + p / up), H = T / 2 = ceil(zeros / s): the weight of
    the input sample k - (H - 1) away from the input base floor(n down / up) of an output n with (n down) mod up = p (the
    layout of ``pk_resample_create``).  s tau is formed as an integer over max(up, down), so the support test is exact."""
    up, down = int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError(f"resample_filter: up = {up}, down = {down} must be positive")
    zeros, rolloff, beta = _filter_params(res_type, zeros, rolloff, beta)
    T = resample_taps(up, down, zeros)
    H = T // 2
    q = (H - 1 - np.arange(T, dtype=np.int64))[None, :] * up + np.arange(up, dtype=np.int64)[:, None]   # tau = q / up
    st = q.astype(np.float64) / float(max(up, down))                                                       # s tau
    inside = np.abs(st) < zeros
    u = np.where(inside, st / zeros, 0.0)
    s = min(1.0, up / down)
    g = s * rolloff * np.sinc(rolloff * st) * np.i0(beta * np.sqrt(1.0 - u * u)) / np.i0(beta)
    return np.where(inside, g, 0.0)


class Resample:
    """``orig_sr`` -> ``target_sr`` on the engine (``pk_resample_*``): y[n] = sum_m x[m] g(n down / up - m) with the filter of
    ``resample_filter``, ceil(N up / down) outputs, zeros outside the signal.  Equal rates return the input as it is (no
    filter, no engine call).  Ragged batches run as one engine call; an utterance's result does not depend on its batch."""

    def __init__(self, orig_sr, target_sr, res_type="kaiser_best", zeros=None, rolloff=None, beta=None, device=None):
        self.orig_sr, self.target_sr = int(orig_sr), int(target_sr)
        self.up, self.down = resample_ratio(orig_sr, target_sr)
        self.zeros, self.rolloff, self.beta = _filter_params(res_type, zeros, rolloff, beta)
        self._device = device
        self.h = None
        self.taps = 0
        if self.up == 1 and self.down == 1:
            return
        self.taps = resample_taps(self.up, self.down, self.zeros)
        _check_resample_envelope(self.up, self.down, self.taps)
        self.ctx = Context.get(device)
        self.table = np.ascontiguousarray(
            resample_filter(self.up, self.down, res_type, self.zeros, self.rolloff, self.beta), dtype=np.float32)
        cfg = _capi.ResampleCfg(self.up, self.down, self.taps)
        h = C.c_void_p()
        _capi.check(self.ctx.lib.pk_resample_create(self.ctx.handle, C.byref(cfg), _capi.fptr(self.table), C.byref(h)))
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.ctx.lib.pk_resample_destroy(h)
            except Exception:
                pass

    def output_length(self, n):
        return -(-int(n) * self.up // self.down)

    @property
    def tile_samples(self):
        """Outputs per workgroup of the engine's kernel (0 for equal rates)."""
        if self.h is None:
            return 0
        t = C.c_int32()
        _capi.check(self.ctx.lib.pk_resample_tile_samples(self.h, C.byref(t)))
        return t.value

    def run_batch(self, wavs):
        """A list of 1-D signals (numpy or tensors) -> a list of (output_length,) device tensors, one engine call."""
        ctx = Context.get(self._device)
        xs = [ctx.to_device(w).reshape(-1) for w in wavs]
        if self.h is None or not xs:
            return [wrap(x) for x in xs]
        lens = np.array([x.numel() for x in xs], dtype=np.int32)
        if lens.min() < 1:
            raise ValueError("Resample: an empty signal")
        x = xs[0] if len(xs) == 1 else torch.cat(xs)
        n_out = [self.output_length(n) for n in lens]
        out = ctx.empty((sum(n_out),))
        _capi.check(ctx.lib.pk_resample_run(self.h, dptr(x), lens.ctypes.data_as(C.POINTER(C.c_int32)), len(xs), dptr(out), 0))
        res, o = [], 0
        for n in n_out:
            res.append(wrap(out[o:o + n]))
            o += n
        return res

    def __call__(self, wav):
        return self.run_batch([wav])[0]


_RESAMPLERS = {}


def _resampler(orig_sr, target_sr, res_type="kaiser_best", zeros=None, rolloff=None, beta=None, device=None):
    """One ``Resample`` per (ratio, filter, device): the table is built and uploaded once."""
    up, down = resample_ratio(orig_sr, target_sr)
    dev = torch.cuda.current_device() if device is None and torch.cuda.is_available() else device
    key = (up, down, res_type, zeros, rolloff, beta, str(dev))
    if key not in _RESAMPLERS:
        _RESAMPLERS[key] = Resample(orig_sr, target_sr, res_type, zeros, rolloff, beta, device)
    return _RESAMPLERS[key]


def resample(y, orig_sr, target_sr, **kw):
    """numpy in, numpy out (float32), on the engine; the argument order of ``librosa.resample``, NOT its filter (see
    ``Resample``).  The last axis is time; leading axes are resampled as a batch.  Equal rates return the samples as they
    are."""
    y = np.asarray(y, dtype=np.float32)
    if resample_ratio(orig_sr, target_sr) == (1, 1):
        return y.copy()
    rs = _resampler(orig_sr, target_sr, **kw)
    if y.ndim == 1:
        return rs(y).cpu().numpy()
    rows = y.reshape(-1, y.shape[-1])
    out = rs.run_batch(list(rows))
    return torch.stack(out).cpu().numpy().reshape(y.shape[:-1] + (-1,))


# ---------------------------------------------------------------------- time stretching and pitch shifting
# csrc/pk_pvoc.h: librosa 0.8's ``phase_vocoder`` restated in float64 without any transcendental function (the accumulated
# phase is a running product of unit phasors), one lane per (utterance, bin); the same bits for an utterance alone, in any
# batch and at any position.  No phase locking: the usual phasiness and the amplitude loss on stretched tones remain.
PVOC_MAX_FRAMES = 1 << 31
PITCH_SHIFT_MAX_DENOMINATOR = 1000
_STRETCH_ENGINES = {}


def _check_rate(rate, what):
    try:
        r = float(rate)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: rate = {rate!r} is not a number") from None
    if not math.isfinite(r) or not r > 0.0:
        raise ValueError(f"{what}: rate = {r} must be finite and > 0")
    return r


def _check_rates(rates, n, what):
    rates = [rates] * n if np.ndim(rates) == 0 else list(rates)
    if len(rates) != n:
        raise ValueError(f"{what}: {len(rates)} rates for {n} utterances; one rate per utterance is needed")
    return [_check_rate(r, what) for r in rates]


def _check_signals(wavs, what):
    wavs = list(wavs)
    if not wavs:
        raise ValueError(f"{what}: no signal given")
    for b, w in enumerate(wavs):
        if not hasattr(w, "shape") or len(w.shape) != 1:
            raise ValueError(f"{what}: signal {b} is not 1-D" + (f" (shape {tuple(w.shape)})" if hasattr(w, "shape") else ""))
        if int(w.shape[0]) < 1:
            raise ValueError(f"{what}: signal {b} is empty")
    return wavs


def pvoc_num_frames(frames, rate):
    """T = ceil(frames / rate) in float64 = ``len(numpy.arange(0, frames, rate))``, from the engine's own function (host only);
    ``ValueError`` for frames < 1, a rate that is not finite or not > 0, T >= 2^31."""
    t = C.c_int64()
    _capi.check(_capi.lib().pk_pvoc_num_frames(int(frames), float(rate), C.byref(t)))
    return t.value


def _pvoc_packed(ctx, x, frames, rates, n_bin):
    """x: the packed (sum(frames), 2 * n_bin) device rows -> (the packed output rows, [T_b]); one engine call."""
    nt = [pvoc_num_frames(f, r) for f, r in zip(frames, rates)]
    out = ctx.empty((sum(nt), 2 * n_bin))
    fr, rt = np.asarray(frames, dtype=np.int32), np.asarray(rates, dtype=np.float64)
    _capi.check(ctx.lib.pk_pvoc_run(ctx.handle, dptr(x), _i32p(fr), len(fr), int(n_bin), rt.ctypes.data_as(C.POINTER(C.c_double)),
                                    dptr(out)))
    return out, nt


def phase_vocoder_batch(specs, rates, device=None):
    """Re-time spectrograms: a ragged list of (frames_b, 2 * n_bin) re | im rows (``pk_mel_run`` what = 0, what
    ``ISTFT.inverse_batch`` takes) and one rate per utterance (or one number for all) -> a list of (T_b, 2 * n_bin) device
    tensors, T_b = ``pvoc_num_frames(frames_b, rate_b)``, in one engine call.  rate > 1 shortens, rate < 1 lengthens."""
    specs = list(specs)
    if not specs:
        raise ValueError("phase_vocoder: no spectrogram given")
    for b, s in enumerate(specs):
        if not hasattr(s, "shape") or len(s.shape) != 2 or s.shape[1] < 2 or s.shape[1] % 2 or s.shape[0] < 1:
            raise ValueError(f"phase_vocoder: spectrogram {b} is not (frames >= 1, 2 * n_bin) re | im rows"
                             + (f" (shape {tuple(s.shape)})" if hasattr(s, "shape") else ""))
        if s.shape[1] != specs[0].shape[1]:
            raise ValueError(f"phase_vocoder: spectrogram {b} has {s.shape[1]} columns, spectrogram 0 has {specs[0].shape[1]}")
    rates = _check_rates(rates, len(specs), "phase_vocoder")
    frames = [int(s.shape[0]) for s in specs]
    for f, r in zip(frames, rates):
        pvoc_num_frames(f, r)                               # T >= 2^31 is refused before a device is needed
    ctx = Context.get(device)
    xs = [ctx.to_device(s) for s in specs]
    out, nt = _pvoc_packed(ctx, xs[0] if len(xs) == 1 else torch.cat(xs), frames, rates, specs[0].shape[1] // 2)
    return [wrap(o) for o in torch.split(out, nt)]


def phase_vocoder(D, rate, hop_length=None, device=None):
    """``librosa.phase_vocoder(D, rate, hop_length)``'s shape: complex (n_bin, frames) -> complex64 (n_bin, T), a numpy array
    for a numpy array and a device tensor for a tensor.  ``hop_length`` is accepted and HAS NO EFFECT: modulo 2 pi the expected
    phase advance it enters is subtracted and added back."""
    del hop_length
    is_t = isinstance(D, torch.Tensor)
    if not hasattr(D, "shape") or len(D.shape) != 2 or D.shape[0] < 1 or D.shape[1] < 1 or not (
            D.is_complex() if is_t else np.iscomplexobj(D)):
        raise ValueError("phase_vocoder: expected a complex (n_bin, frames) spectrogram"
                         + (f", got shape {tuple(D.shape)}" if hasattr(D, "shape") else ""))
    rate = _check_rate(rate, "phase_vocoder")
    if is_t:
        D = D.as_subclass(torch.Tensor)
        rows = torch.cat([D.real, D.imag], 0).transpose(0, 1).to(torch.float32)
    else:
        rows = np.ascontiguousarray(np.concatenate([D.real.T, D.imag.T], axis=1), dtype=np.float32)
    out = phase_vocoder_batch([rows], [rate], device)[0].as_subclass(torch.Tensor)
    nb = D.shape[0]
    res = torch.complex(out[:, :nb], out[:, nb:]).transpose(0, 1)
    return wrap(res.contiguous()) if is_t else res.cpu().numpy()


def _stretch_engines(n_fft, hop_length, win_length, window, transform, device=None):
    """The forward and the inverse STFT handle of one configuration (center=True, reflect padding), created once."""
    ctx = Context.get(device)
    key = (int(n_fft), int(hop_length), int(win_length), window, transform, str(ctx.device))
    if key not in _STRETCH_ENGINES:
        _STRETCH_ENGINES[key] = (_Engine(n_fft, hop_length, win_length, window, True, False, None, 0, device, transform),
                                 _InvEngine(n_fft, hop_length, win_length, window, True, device, transform))
    return _STRETCH_ENGINES[key]


def stretched_length(n, rate):
    """``int(round(n / rate))``, librosa's ``len_stretch``.  Python's ``round`` takes a tie to the EVEN integer (2.5 -> 2,
    3.5 -> 4), and so does this."""
    return int(round(int(n) / float(rate)))


def _fit_length(y, n):
    """Crop or zero-pad a 1-D device tensor to n samples (librosa's ``fix_length``)."""
    if y.numel() >= n:
        return y[:n]
    return torch.cat([y, torch.zeros(n - y.numel(), dtype=y.dtype, device=y.device)])


def time_stretch_batch(wavs, rates, n_fft=2048, hop_length=None, win_length=None, window="hann", transform="dense", device=None):
    """``librosa.effects.time_stretch`` for a ragged list of float32 signals, one rate per utterance (or one number for all):
    STFT (center=True, reflect padding) -> phase vocoder -> ISTFT as three engine calls with nothing read back in between; frame
    counts and lengths follow from the input lengths on the host.  Each result is cropped or zero-padded to
    ``stretched_length(len(y), rate)`` samples.  ``hop_length`` defaults to ``n_fft // 4``.  rate > 1 is faster and shorter.
    A list of device tensors.  n_fft must be a multiple of 16 and hop_length of 4, ``transform="fft"`` takes powers of two from
    32 to 4096, a signal must be longer than ``n_fft // 2`` samples: the STFT's and ISTFT's own errors say so."""
    wavs = _check_signals(wavs, "time_stretch")
    rates = _check_rates(rates, len(wavs), "time_stretch")
    _transform_id(transform)
    n_fft = int(n_fft)
    hop_length = n_fft // 4 if hop_length is None else int(hop_length)
    win_length = n_fft if win_length is None else int(win_length)
    fwd, inv = _stretch_engines(n_fft, hop_length, win_length, window, transform, device)
    ctx = Context.get(device)
    lens, x = _pack_ragged(ctx, wavs, "time_stretch")
    B, nb = len(lens), fwd.n_bin
    nf = [fwd.frames(n) for n in lens]
    spec = ctx.empty((sum(nf), 2 * nb))
    _capi.check(ctx.lib.pk_mel_run(fwd.h, dptr(x), _i32p(lens), B, dptr(spec), 0, 0))
    rows, nt = _pvoc_packed(ctx, spec, nf, rates, nb)
    ns = [inv.samples(t) for t in nt]
    y = ctx.empty((max(1, sum(ns)),))
    _capi.check(ctx.lib.pk_istft_run(inv.h, dptr(rows), _i32p(np.asarray(nt, dtype=np.int32)), B, dptr(y), 0))
    return [wrap(_fit_length(p, stretched_length(n, r))) for p, n, r in zip(torch.split(y[:sum(ns)], ns), lens, rates)]


def time_stretch(y, rate, **kw):
    return time_stretch_batch([y], [rate], **kw)[0]


def pitch_shift_ratio(n_steps, bins_per_octave=12):
    """(Fraction, cents_off): the rational nearest the stretch rate ``2 ** (-n_steps / bins_per_octave)`` with a denominator of
    at most 1000 (``Fraction.limit_denominator``), and how far the shift it realises is from the one asked for, in cents
    (positive: sharp).  Exact for whole octaves; within 0.027 cent for every integer step within two octaves at 12 and 24 bins
    per octave."""
    if int(bins_per_octave) != bins_per_octave or bins_per_octave < 1:
        raise ValueError(f"pitch_shift: bins_per_octave = {bins_per_octave!r} must be a positive integer")
    try:
        steps = float(n_steps)
    except (TypeError, ValueError):
        raise ValueError(f"pitch_shift: n_steps = {n_steps!r} is not a number") from None
    if not math.isfinite(steps):
        raise ValueError(f"pitch_shift: n_steps = {steps} must be finite")
    try:
        rate = 2.0 ** (-steps / int(bins_per_octave))
    except OverflowError:
        rate = math.inf
    if not math.isfinite(rate) or not rate > 0.0:
        raise ValueError(f"pitch_shift: n_steps = {steps} at {bins_per_octave} bins per octave is no usable ratio")
    fr = Fraction(rate).limit_denominator(PITCH_SHIFT_MAX_DENOMINATOR)
    if fr <= 0:
        raise ValueError(f"pitch_shift: n_steps = {steps} at {bins_per_octave} bins per octave is no usable ratio")
    return fr, 1200.0 * math.log2(rate / (fr.numerator / fr.denominator))


def pitch_shift_batch(wavs, sr, n_steps, bins_per_octave=12, res_type="kaiser_best", device=None, **stft_kw):
    """``librosa.effects.pitch_shift`` for a ragged list of signals, one shift for the batch: a time stretch by the rational rate
    p / q of ``pitch_shift_ratio`` and then ``audio.Resample`` at that same ratio (up / down = p / q in lowest terms: librosa's
    ``resample(orig_sr=sr / rate, target_sr=sr)``), each result cropped or zero-padded to its input's length.  The resampler is
    THIS PROJECT'S filter, not librosa's.  ``sr`` enters no arithmetic (the ratio does not depend on it); it is
    checked.  ``n_steps = 0`` returns the inputs as they are, without an engine call; a ratio outside ``Resample``'s envelope
    raises its ``NotImplementedError``.  ``stft_kw``: n_fft, hop_length, win_length, window, transform of ``time_stretch``."""
    wavs = _check_signals(wavs, "pitch_shift")
    if not (isinstance(sr, (int, float, np.integer, np.floating)) and math.isfinite(sr) and sr > 0):
        raise ValueError(f"pitch_shift: sr = {sr!r} must be a positive number")
    fr, _ = pitch_shift_ratio(n_steps, bins_per_octave)
    if float(n_steps) == 0.0:
        ctx = Context.get(device)
        return [wrap(ctx.to_device(w)) for w in wavs]
    rs = _resampler(fr.denominator, fr.numerator, res_type=res_type, device=device)        # the envelope is checked here
    out = rs.run_batch(time_stretch_batch(wavs, fr.numerator / fr.denominator, device=device, **stft_kw))
    return [wrap(_fit_length(o.as_subclass(torch.Tensor), int(w.shape[0]))) for o, w in zip(out, wavs)]


def pitch_shift(y, sr, n_steps, bins_per_octave=12, res_type="kaiser_best", **kw):
    return pitch_shift_batch([y], sr, n_steps, bins_per_octave, res_type, **kw)[0]


def _decode_wav(data):
    """RIFF/WAVE bytes -> ((frames, channels) samples, rate, bits, is_float); integer PCM of 8, 16, 24, 32 bits, IEEE float32,
    plain or WAVE_FORMAT_EXTENSIBLE."""
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    pos, fmt, body = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        chunk = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = chunk
        elif cid == b"data":
            body = chunk
            break
        pos += 8 + size + (size & 1)
    if fmt is None or body is None or len(fmt) < 16:
        raise ValueError("no fmt / data chunk")
    tag, ch, rate, _, block, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE and len(fmt) >= 26:
        tag = struct.unpack("<H", fmt[24:26])[0]            # the sub-format GUID starts with the plain format tag
    if ch < 1 or rate < 1:
        raise ValueError(f"{ch} channels at {rate} Hz")
    if (tag, bits) not in ((1, 8), (1, 16), (1, 24), (1, 32), (3, 32)):
        raise NotImplementedError(f"format tag {tag} with {bits} bits per sample (integer PCM of 8 / 16 / 24 / 32 bits and "
                                  "32-bit float are read)")
    width = bits // 8
    body = body[:len(body) // (width * ch) * (width * ch)]
    if tag == 3:
        x = np.frombuffer(body, dtype="<f4")
    elif bits == 8:
        x = np.frombuffer(body, dtype=np.uint8).astype(np.int16) - 128
    elif bits == 16:
        x = np.frombuffer(body, dtype="<i2")
    elif bits == 32:
        x = np.frombuffer(body, dtype="<i4")
    else:
        b = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        x = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16))
        x = x - ((x & 0x800000) << 1)
    return x.reshape(-1, ch), rate, bits, tag == 3


def load_wav(path, sr=None, mono=True, res_type="kaiser_best"):
    """(float32 wav, sampling rate) of a RIFF/WAVE file: the ``librosa.load(path, sr=fs)`` the reference's feature recipes begin
    with (examples/fastspeech2/preprocess.py:54-55), with this project's resampler in place of librosa's.  Integer samples are
    divided by 2^(bits - 1); ``mono`` averages the channels, otherwise the result is (channels, T) for a file of several.
    ``sr``: None keeps the file's rate; another rate resamples on the engine (``Resample``).  ``path`` may be bytes."""
    if isinstance(path, (bytes, bytearray)):
        data = bytes(path)
    elif hasattr(path, "read"):
        data = path.read()
    else:
        with open(path, "rb") as f:
            data = f.read()
    try:
        x, rate, bits, is_float = _decode_wav(data)
    except (ValueError, NotImplementedError) as e:
        raise type(e)(f"{path if not isinstance(path, (bytes, bytearray)) else '<bytes>'}: {e}") from None
    acc = np.float64 if bits == 32 and not is_float else np.float32       # 24 bits are exact in float32, 32 are not
    x = x.astype(acc)
    x = x.mean(axis=1) if mono or x.shape[1] == 1 else np.ascontiguousarray(x.T)
    if not is_float:
        x = x / acc(1 << (bits - 1))
    wav = x.astype(np.float32, copy=False)
    if sr is not None and int(sr) != rate:
        wav = resample(wav, rate, sr, res_type=res_type)
        rate = int(sr)
    return wav, rate


def wav_bytes(wav, samplerate, subtype="PCM_16", source_samplerate=None):
    """The bytes ``write_wav`` puts into the file (a serving process sends them instead of writing a file)."""
    import io
    buf = io.BytesIO()
    write_wav(buf, wav, samplerate, subtype, source_samplerate)
    return buf.getvalue()


def write_wav(path, wav, samplerate, subtype="PCM_16", source_samplerate=None):
    """Minimal stand-in for the ``soundfile.write(path, wav.numpy(), samplerate=fs)`` at the end of the
    synthesis recipes (examples/fastspeech2/ljspeech/synthesize_e2e.py:104-107): RIFF/WAVE, mono or
    (T, C) float input in [-1, 1].  "PCM_16" (libsndfile's default for .wav: clip, scale by 32767, round to
    nearest) or "FLOAT" (32-bit IEEE samples, lossless).  ``source_samplerate``: the rate ``wav`` is at, when the file is to
    be at another one (``samplerate``): it is resampled on the engine (``Resample``) before it is encoded."""
    x = np.asarray(wav.cpu() if isinstance(wav, torch.Tensor) else wav, dtype=np.float32)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2:
        raise ValueError("write_wav: expected (T,) or (T, channels)")
    if source_samplerate is not None and int(source_samplerate) != int(samplerate):
        x = np.ascontiguousarray(resample(np.ascontiguousarray(x.T), source_samplerate, samplerate).T)
    n, ch = x.shape
    if subtype == "PCM_16":
        data = np.rint(np.clip(x, -1.0, 1.0) * 32767.0).astype("<i2").tobytes()
        fmt, bits = 1, 16
    elif subtype == "FLOAT":
        data = x.astype("<f4").tobytes()
        fmt, bits = 3, 32
    else:
        raise ValueError(f"write_wav: unsupported subtype {subtype!r}")
    block = ch * bits // 8
    header = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack(
        "<IHHIIHH", 16, fmt, ch, int(samplerate), int(samplerate) * block, block, bits) + b"data" + struct.pack(
        "<I", len(data))
    if hasattr(path, "write"):       # a binary file object (wav_bytes)
        path.write(header)
        path.write(data)
        return
    with open(path, "wb") as f:
        f.write(header)
        f.write(data)


def stft(x, fft_size, hop_length=None, win_length=None, window="hann", center=True, pad_mode="reflect"):
    """``parakeet.modules.stft_loss.stft`` (:20-67): (B, T) -> magnitude spectrogram (B, frames, fft_size//2+1),
    ``sqrt(clip(re^2 + im^2, min=1e-7))``.  The transform runs on the engine (STFT-as-GEMM + magnitude kernel);
    the floor is one elementwise maximum with sqrt(1e-7) on the result."""
    win_length = win_length or fft_size
    t = STFT(fft_size, hop_length, win_length, window, center, pad_mode)
    mag = t.magnitude(x).as_subclass(torch.Tensor)                    # (B, bins, frames)
    return wrap(torch.clamp_min(mag, float(np.sqrt(np.float32(1e-7)))).transpose(1, 2).contiguous())


class LogMagnitude:
    """parakeet/audio/spec_normalizer.py:37-53 (the WaveFlow / Tacotron2 feature domain): log(max(x, min))."""

    def __init__(self, min=1e-5):   # noqa: A002  (the reference's argument name)
        self.min = min

    def transform(self, x):
        return np.log(np.maximum(np.asarray(x), self.min))

    def inverse(self, x):
        return np.exp(np.asarray(x))


class UnitMagnitude:
    """parakeet/audio/spec_normalizer.py:56-75: dB scale mapped to [0, 1] (20 log10(max(x, min)) - 20, then (. + 100) / 100,
    clipped) and back.  Host-side numpy, like the reference."""

    def __init__(self, min=1e-5):   # noqa: A002
        self.min = min

    def transform(self, x):
        db = 20.0 * np.log10(np.maximum(self.min, np.asarray(x))) - 20.0
        return np.clip((db + 100.0) / 100.0, 0, 1)

    def inverse(self, x):
        db = np.clip(np.asarray(x), 0, 1) * 100.0 - 100.0
        return np.exp((db + 20.0) / 20.0 * np.log(10))


class AudioProcessor:
    """parakeet/audio/audio.py:20-102 with the transforms on the engine: ``spectrogram`` = |STFT|,
    ``mel_spectrogram`` = mel_filter . |STFT| (the Slaney filterbank of ``librosa.filters.mel``), both returned
    as (bins, frames) numpy arrays like the reference.  ``read_wav`` reads PCM / float RIFF files (``load_wav``); a file at
    another rate is resampled to the processor's on the engine, where the reference resamples with librosa."""

    def __init__(self, sample_rate, n_fft, win_length, hop_length, n_mels=80, fmin=0, fmax=None, window="hann",
                 center=True, pad_mode="reflect", normalize=True, transform="dense"):
        if pad_mode != "reflect":
            raise NotImplementedError("only pad_mode='reflect' is implemented")
        self.transform = transform
        self.sample_rate, self.normalize = sample_rate, normalize
        self.n_fft, self.win_length, self.hop_length = n_fft, win_length, hop_length
        self.window, self.center, self.pad_mode = window, center, pad_mode
        self.n_mels, self.fmin, self.fmax = n_mels, fmin, fmax
        self.mel_filter = mel_filterbank(sample_rate, n_fft, n_mels, fmin or 0, fmax or sample_rate / 2)
        self.inv_mel_filter = np.linalg.pinv(self.mel_filter)
        self._spec = _Engine(n_fft, hop_length, win_length, window, center, False, None, 0, transform=transform)
        self._mel = _Engine(n_fft, hop_length, win_length, window, center, False, self.mel_filter, 0, transform=transform)
        self._inv = None

    def read_wav(self, filename):
        wav, _ = load_wav(filename, sr=self.sample_rate)
        if self.normalize:
            wav = wav / np.max(np.abs(wav)) * 0.999
        return wav

    def write_wav(self, path, wav):
        write_wav(path, wav, self.sample_rate)

    def spectrogram(self, wav):
        return self._spec.run([np.asarray(wav, dtype=np.float32)], 1)[0].cpu().numpy().T

    def mel_spectrogram(self, wav):
        return self._mel.run([np.asarray(wav, dtype=np.float32)], 2)[0].cpu().numpy().T

    def stft(self, wav):
        """complex64 (n_bin, frames), audio.py:75-84."""
        o = self._spec.run([np.asarray(wav, dtype=np.float32)], 0)[0].cpu().numpy()
        nb = self._spec.n_bin
        return (o[:, :nb] + 1j * o[:, nb:]).T.astype(np.complex64)

    def _inverse(self):
        if self._inv is None:
            self._inv = _InvEngine(self.n_fft, self.hop_length, self.win_length, self.window, self.center,
                                   transform=self.transform)
        return self._inv

    @staticmethod
    def _reim_rows(D):
        D = np.asarray(D)
        return np.ascontiguousarray(np.concatenate([D.real.T, D.imag.T], axis=1), dtype=np.float32)

    def istft(self, D):
        """complex (n_bin, frames) -> float32 (T,), audio.py:86-93."""
        return self._inverse().run([self._reim_rows(D)])[0].cpu().numpy()

    def griffin_lim_batch(self, specs, n_iter=32, momentum=0.99, seeds=None, angles=None):
        """Ragged ``griffin_lim``: a list of (n_bin, frames_b) magnitudes (and complex initial phases) -> list of (T_b,)."""
        ctx = Context.get()
        mags = [ctx.to_device(S).transpose(0, 1) for S in specs]
        ang = None if angles is None else [self._reim_rows(a) for a in angles]
        out = self._inverse().griffin_lim(self._spec, mags, n_iter, momentum, seeds, ang)
        return [o.cpu().numpy() for o in out]

    def griffin_lim(self, S, n_iter=32, momentum=0.99, seed=0, angles=None):
        """``librosa.griffinlim`` on the engine: S (n_bin, frames) magnitudes as ``spectrogram`` returns them -> float32
        (T,).  ``angles``: complex (n_bin, frames) initial phases of unit modulus; None draws them from ``seed``."""
        return self.griffin_lim_batch([S], n_iter, momentum, [seed], None if angles is None else [angles])[0]

    def _mel_to_linear_rows(self, x):
        """(rows, n_mels) device -> (rows, n_bin) device: one engine GEMM over frames and the floor."""
        ctx = Context.get()
        if x.dim() != 2 or x.shape[1] != self.n_mels:
            raise AssertionError(f"mel_to_linear: expected {self.n_mels} mel bins, got {tuple(x.shape)}")
        nb = self.inv_mel_filter.shape[0]
        y = ctx.empty((x.shape[0], nb))
        wkn = np.ascontiguousarray(self.inv_mel_filter.T, dtype=np.float32)        # [n_mels][n_bin]
        _capi.check(ctx.lib.pk_op_matmul(ctx.handle, dptr(x), x.shape[0], self.n_mels, nb, _capi.fptr(wkn), None, dptr(y)))
        return torch.clamp_min(y, 1e-10)

    def mel_to_linear(self, mel):
        """``maximum(1e-10, inv_mel_filter @ mel)``: (n_mels, frames) -> (n_bin, frames) numpy."""
        x = Context.get().to_device(mel)
        if x.dim() != 2:
            raise AssertionError(f"mel_to_linear: expected (n_mels, frames), got {tuple(x.shape)}")
        return self._mel_to_linear_rows(x.transpose(0, 1).contiguous()).cpu().numpy().T


class GriffinLim:
    """A weight-free vocoder: mel -> ``spec_normalizer.inverse`` -> ``mel_to_linear`` -> ``** power`` -> Griffin-Lim.
    ``spec_normalizer`` is e.g. ``LogMagnitude()`` for the Tacotron2 / TransformerTTS / WaveFlow feature domain (its inverse
    is a plain exp); None takes the mel as linear magnitudes."""

    def __init__(self, audio_processor, spec_normalizer=None, n_iter=32, momentum=0.99, power=1.0):
        self.audio_processor, self.spec_normalizer = audio_processor, spec_normalizer
        self.n_iter, self.momentum, self.power = n_iter, momentum, power

    def infer_batch(self, mels, seeds=None):
        """A list of (n_mels, frames_b) -> a list of float32 (T_b,); ``seeds``: one integer per utterance (default 0)."""
        ap, ctx = self.audio_processor, Context.get()
        mels = [np.asarray(m.cpu() if isinstance(m, torch.Tensor) else m, dtype=np.float32) for m in mels]
        for m in mels:
            if m.ndim != 2 or m.shape[0] != ap.n_mels:
                raise AssertionError(f"GriffinLim: expected ({ap.n_mels}, frames) mels, got {m.shape}")
        if self.spec_normalizer is not None:
            mels = [np.asarray(self.spec_normalizer.inverse(m), dtype=np.float32) for m in mels]
        lin = ap._mel_to_linear_rows(ctx.to_device(np.concatenate([m.T for m in mels], axis=0)))   # one GEMM for the batch
        if self.power != 1.0:
            lin = torch.pow(lin, float(self.power))
        specs, o = [], 0
        for m in mels:
            specs.append(lin[o:o + m.shape[1]].transpose(0, 1))
            o += m.shape[1]
        return ap.griffin_lim_batch(specs, self.n_iter, self.momentum, seeds)

    def infer(self, mel, seed=0):
        """(n_mels, frames) -> (T,), or (B, n_mels, frames) -> (B, T)."""
        mel = np.asarray(mel.cpu() if isinstance(mel, torch.Tensor) else mel, dtype=np.float32)
        if mel.ndim == 2:
            return self.infer_batch([mel], [seed])[0]
        return np.stack(self.infer_batch(list(mel), [seed] * mel.shape[0]))

    __call__ = infer
