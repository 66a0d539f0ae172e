"""Multi-resolution STFT loss behind the reference's Python API, at any hop length.

Mirrors parakeet/modules/stft_loss.py: ``stft`` (:20-67), ``SpectralConvergenceLoss`` (:70-92), ``LogSTFTMagnitudeLoss``
(:95-118), ``STFTLoss`` (:121-160) and ``MultiResolutionSTFTLoss`` (:163-219), the two numbers the Parallel WaveGAN evaluator
reports as ``eval/spectral_convergence_loss`` and ``eval/log_stft_magnitude_loss`` (parallel_wavegan_updater.py:204-211).
Inference only: no gradients.

The arithmetic runs in libpk_synth.so (csrc/stft_dist.hip): the transform of both signals at every resolution, the
magnitudes, the three terms and their sums per utterance.  ``pk_stftd_run`` returns ``(B, R, 3)`` float64 sums
``sum (Y - X)^2``, ``sum Y^2``, ``sum |ln Y - ln X|``; the two losses are formed from them here, on the host, in float64.
Unlike ``parakeet_amd.audio.stft`` the hop is any integer >= 1 (the reference's third resolution is 512 / 50 / 240).
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _capi
from .audio import _window
from .runtime import Context, dptr, wrap

POWER_FLOOR = 1e-7     # stft_loss.py:66  clip(real**2 + imag**2, min=1e-7)
LOG_FLOOR = 1e-7       # stft_loss.py:98  LogSTFTMagnitudeLoss(epsilon=1e-7)
NORM_FLOOR = 1e-10     # stft_loss.py:92  clip(norm(y_mag), min=1e-10)


class _DistEngine:
    """A pk_stftd handle: R resolutions (n_fft, hop, win_length), one window name, one centring."""

    def __init__(self, fft_sizes, hop_sizes, win_lengths, window="hann", center=True, log_floor=LOG_FLOOR, device=None):
        if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)) or len(fft_sizes) == 0:
            raise AssertionError("fft_sizes, hop_sizes and win_lengths must have one entry per resolution")
        self.ctx = Context.get(device)
        R = len(fft_sizes)
        self.resolutions = [(int(n), int(h), int(w)) for n, h, w in zip(fft_sizes, hop_sizes, win_lengths)]
        self.n_bins = [1 + n // 2 for n, _, _ in self.resolutions]
        for n, _, w in self.resolutions:
            if w > n:
                raise AssertionError(f"win_length {w} exceeds fft_size {n}")
        res = (_capi.StftdRes * R)(*[_capi.StftdRes(n, h, 1 if center else 0) for n, h, _ in self.resolutions])
        wins = np.ascontiguousarray(np.concatenate([_window(window, w, n) for n, _, w in self.resolutions]), np.float32)
        cfg = _capi.StftdCfg(R, POWER_FLOOR, float(log_floor))
        h = C.c_void_p()
        _capi.check(self.ctx.lib.pk_stftd_create(self.ctx.handle, C.byref(cfg), res, _capi.fptr(wins), C.byref(h)))
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.ctx.lib.pk_stftd_destroy(h)
            except Exception:
                pass

    def frames(self, r, n):
        f = C.c_int32()
        _capi.check(self.ctx.lib.pk_stftd_num_frames(self.h, int(r), int(n), C.byref(f)))
        return f.value

    def _pack(self, wavs):
        ctx = Context.get(self.ctx.device)
        sig = [ctx.to_device(w).reshape(-1) for w in wavs]
        lens = np.array([s.numel() for s in sig], dtype=np.int32)
        return ctx, (torch.cat(sig) if len(sig) > 1 else sig[0]), lens

    def sums(self, xs, ys):
        """Two lists of 1-D signals, pairwise of equal length -> (B, R, 3) float64 numpy."""
        if len(xs) != len(ys):
            raise ValueError(f"{len(xs)} predicted signals against {len(ys)} ground-truth signals")
        if len(xs) == 0:
            raise ValueError("no signals given")
        ctx, x, lens = self._pack(xs)
        _, y, ylens = self._pack(ys)
        if not np.array_equal(lens, ylens):
            b = int(np.nonzero(lens != ylens)[0][0])
            raise ValueError(f"pair {b}: predicted signal has {lens[b]} samples, ground truth {ylens[b]}")
        out = ctx.empty((len(xs), len(self.resolutions), 3), dtype=torch.float64)
        _capi.check(ctx.lib.pk_stftd_run(self.h, dptr(x), dptr(y), lens.ctypes.data_as(C.POINTER(C.c_int32)), len(xs),
                                         dptr(out), 0))
        return out.cpu().numpy()

    def magnitude(self, r, wavs):
        """List of 1-D signals -> list of (frames, n_bin) device tensors of resolution r."""
        if len(wavs) == 0:
            raise ValueError("no signals given")
        ctx, x, lens = self._pack(wavs)
        nf = [self.frames(r, n) for n in lens]
        out = ctx.empty((max(1, sum(nf)), self.n_bins[r]))
        _capi.check(ctx.lib.pk_stftd_magnitude(self.h, int(r), dptr(x), lens.ctypes.data_as(C.POINTER(C.c_int32)),
                                               len(wavs), dptr(out), 0))
        res, o = [], 0
        for f in nf:
            res.append(out[o:o + f])
            o += f
        return res

    def entries(self, lens):
        """(B, R) number of frames x n_bin entries behind each sum."""
        return np.array([[self.frames(r, n) * self.n_bins[r] for r in range(len(self.resolutions))] for n in lens],
                        dtype=np.float64)


def losses_from_sums(sums, entries):
    """(..., 3) sums over any set of entries and their count -> (sc_loss, mag_loss), float64:
    sqrt(sum (Y - X)^2) / max(sqrt(sum Y^2), 1e-10) and sum |ln Y - ln X| / entries.  A count of zero (an uncentred
    transform longer than the signal) raises ValueError."""
    sums = np.asarray(sums, np.float64)
    if not np.all(np.asarray(entries) > 0):
        raise ValueError("a signal is shorter than one frame of a resolution: there is nothing to average")
    sc = np.sqrt(sums[..., 0]) / np.maximum(np.sqrt(sums[..., 1]), NORM_FLOOR)
    return sc, sums[..., 2] / np.asarray(entries, np.float64)


_ENGINES = collections.OrderedDict()
MAX_CACHED_ENGINES = 4     # a handle keeps its bases and grow-only workspaces on the device


def _engine(fft_sizes, hop_sizes, win_lengths, window, center=True, log_floor=LOG_FLOOR):
    """The handle for these parameters, from a cache of the MAX_CACHED_ENGINES most recently used ones (``stft`` is a
    function: without the cache every call would build its basis again).  A handle that leaves the cache is destroyed,
    with its device memory, once no loss object holds it."""
    ctx = Context.get()
    key = (ctx.device.index, tuple(fft_sizes), tuple(hop_sizes), tuple(win_lengths), window, bool(center), float(log_floor))
    if key in _ENGINES:
        _ENGINES.move_to_end(key)
    else:
        _ENGINES[key] = _DistEngine(fft_sizes, hop_sizes, win_lengths, window, center, log_floor)
        while len(_ENGINES) > MAX_CACHED_ENGINES:
            _ENGINES.popitem(last=False)
    return _ENGINES[key]


def clear_cache():
    """Drop the cached handles (and the device memory of those no loss object holds)."""
    _ENGINES.clear()


def _rows(x):
    """(B, T) or (B, C, T) -> (B x C, T) torch tensor (stft_loss.py:205-209)."""
    x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    x = x.as_subclass(torch.Tensor)
    if x.dim() == 3:
        x = x.reshape(-1, x.shape[2])
    if x.dim() != 2:
        raise AssertionError(f"expected (B, T) or (B, C, T), got {tuple(x.shape)}")
    return x


def stft(x, fft_size, hop_length=None, win_length=None, window="hann", center=True, pad_mode="reflect"):
    """``parakeet.modules.stft_loss.stft`` (:20-67): (B, T) -> (B, frames, fft_size // 2 + 1),
    ``sqrt(clip(re^2 + im^2, min=1e-7))``, at any hop length (``pk_stftd_magnitude``)."""
    if pad_mode != "reflect":
        raise NotImplementedError("only pad_mode='reflect' is implemented")
    win_length = win_length or fft_size
    hop_length = hop_length or int(win_length // 4)
    x = _rows(x)
    eng = _engine([fft_size], [hop_length], [win_length], window, center)
    outs = eng.magnitude(0, [x[b] for b in range(x.shape[0])])
    return wrap(torch.stack(outs, 0))


class SpectralConvergenceLoss:
    """``norm(y_mag - x_mag, "fro") / clip(norm(y_mag, "fro"), 1e-10)`` of given magnitudes (:70-92), on their device."""

    def forward(self, x_mag, y_mag):
        x = torch.as_tensor(x_mag).as_subclass(torch.Tensor)
        y = torch.as_tensor(y_mag).as_subclass(torch.Tensor)
        return wrap(torch.linalg.vector_norm(y - x) / torch.clamp_min(torch.linalg.vector_norm(y), NORM_FLOOR))

    __call__ = forward


class LogSTFTMagnitudeLoss:
    """``l1_loss(log(clip(y_mag, eps)), log(clip(x_mag, eps)))`` of given magnitudes (:95-118), on their device."""

    def __init__(self, epsilon=1e-7):
        self.epsilon = epsilon

    def forward(self, x_mag, y_mag):
        x = torch.as_tensor(x_mag).as_subclass(torch.Tensor)
        y = torch.as_tensor(y_mag).as_subclass(torch.Tensor)
        return wrap(torch.mean(torch.abs(torch.log(torch.clamp_min(y, self.epsilon)) -
                                         torch.log(torch.clamp_min(x, self.epsilon)))))

    __call__ = forward


class MultiResolutionSTFTLoss:
    """(x, y) -> (sc_loss, mag_loss), each the mean over the resolutions of the batch-global loss (:163-219)."""

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240), window="hann"):
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths)
        self.fft_sizes, self.hop_sizes, self.win_lengths = list(fft_sizes), list(hop_sizes), list(win_lengths)
        self.window = window
        self._eng = _engine(self.fft_sizes, self.hop_sizes, self.win_lengths, window)

    def resolution_losses(self, x, y):
        """(B, T) or (B, C, T) -> two (R,) float64 arrays: the batch-global losses of each resolution."""
        x, y = _rows(x), _rows(y)
        if x.shape != y.shape:
            raise ValueError(f"predicted signals {tuple(x.shape)} against ground truth {tuple(y.shape)}")
        B = x.shape[0]
        sums = self._eng.sums([x[b] for b in range(B)], [y[b] for b in range(B)])
        entries = self._eng.entries([x.shape[1]] * B)
        return losses_from_sums(sums.sum(0), entries.sum(0))

    def forward(self, x, y):
        sc, mag = self.resolution_losses(x, y)
        dev = Context.get().device
        return (wrap(torch.tensor(sc.mean(), dtype=torch.float32, device=dev)),
                wrap(torch.tensor(mag.mean(), dtype=torch.float32, device=dev)))

    __call__ = forward

    def per_utterance(self, xs, ys):
        """Ragged lists of 1-D signals -> (B, R, 2) float64 numpy: (sc_loss, mag_loss) of every pair at every resolution,
        each pair scored as the reference would score a batch of one.  Pairs of unequal length, or lists of unequal
        size, raise ValueError."""
        xs, ys = list(xs), list(ys)
        sums = self._eng.sums(xs, ys)
        entries = self._eng.entries([int(np.prod(tuple(w.shape))) for w in xs])
        sc, mag = losses_from_sums(sums, entries)
        return np.stack([sc, mag], -1)


class STFTLoss(MultiResolutionSTFTLoss):
    """One resolution (:121-160)."""

    def __init__(self, fft_size=1024, shift_size=120, win_length=600, window="hann"):
        super().__init__([fft_size], [shift_size], [win_length], window)
        self.fft_size, self.shift_size, self.win_length = fft_size, shift_size, win_length
        self.spectral_convergence_loss = SpectralConvergenceLoss()
        self.log_stft_magnitude_loss = LogSTFTMagnitudeLoss()
