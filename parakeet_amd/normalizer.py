"""ZScore normaliser with the reference's interface (parakeet/modules/normalizer.py:18-33).

Inside the engine the two affines are fused into the kernels that produce /
consume the mel (FastSpeech2Inference output, PWGInference input); this class
carries the statistics and offers forward/inverse on host or device arrays.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, to_numpy_f32


class ZScore:
    # feature last
    def __init__(self, mu, sigma):
        self.mu = to_numpy_f32(mu)
        self.sigma = to_numpy_f32(sigma)

    def _stats(self, x):
        if isinstance(x, torch.Tensor):
            return (torch.as_tensor(self.mu, device=x.device), torch.as_tensor(self.sigma, device=x.device))
        return self.mu, self.sigma

    def forward(self, x):
        mu, sigma = self._stats(x)
        return (x - mu) / sigma

    __call__ = forward

    def inverse(self, x):
        mu, sigma = self._stats(x)
        return x * sigma + mu

    @classmethod
    def from_stats(cls, stats):
        """From the (2, D) array [mean, scale] that ``FeatureStats.save`` and the reference's compute_statistics.py write,
        or the path of its .npy file."""
        if isinstance(stats, (str, bytes, os.PathLike)):
            stats = np.load(stats, allow_pickle=False)
        stats = np.asarray(stats.detach().cpu().numpy() if isinstance(stats, torch.Tensor) else stats)
        if stats.ndim != 2 or stats.shape[0] != 2:
            raise ValueError(f"statistics are a (2, D) array [mean, scale], got shape {stats.shape}")
        return cls(stats[0], stats[1])


# ---- feature statistics ----------------------------------------------------------------------------------------------
# DESIGN.md 4.5g; the definition and THE ORDER of every sum: csrc/pk_stats.h.  What the reference's utils/compute_statistics.py
# takes from scikit-learn's StandardScaler.partial_fit (scikit-learn is not a dependency).
_F64_EPS = float(np.finfo(np.float64).eps)


def derive_stats(n, shift, s1, s2):
    """(mean, var, scale) in float64 from a state: mean = K + S1 / n, var = max(S2 - S1^2 / n, 0) / n (population variance),
    scale = sqrt(var), replaced by 1 where scikit-learn's constant-feature test holds (``_is_constant_feature``:
    var <= n eps var + (n mean eps)^2 with eps = 2^-52; ``_handle_zeros_in_scale`` then sets those scales to 1)."""
    n = int(n)
    if n < 1:
        raise RuntimeError("FeatureStats has seen no rows yet")
    nf = np.float64(n)
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    mean = np.asarray(shift, np.float32).astype(np.float64) + s1 / nf
    var = np.maximum(s2 - s1 * s1 / nf, 0.0) / nf
    scale = np.sqrt(var)
    constant = var <= nf * _F64_EPS * var + (nf * mean * _F64_EPS) ** 2
    scale[constant] = 1.0
    return mean, var, scale


def reshift(n, shift_from, s1, s2, shift_to):
    """(S1, S2) of the same n rows about another shift, in float64: with delta = K_from - K_to,
    S1' = S1 + n delta, S2' = S2 + 2 delta S1 + n delta^2."""
    delta = np.asarray(shift_from, np.float32).astype(np.float64) - np.asarray(shift_to, np.float32).astype(np.float64)
    nf = np.float64(int(n))
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    return s1 + nf * delta, s2 + 2.0 * delta * s1 + nf * delta * delta


class _StatsEngine:
    """One ``pk_stats`` handle."""

    def __init__(self, dim, device=None):
        self.ctx = Context.get(device)
        h = C.c_void_p()
        _capi.check(self.ctx.lib.pk_stats_create(self.ctx.handle, int(dim), C.byref(h)))
        self.h = h

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.ctx.lib.pk_stats_destroy(h)
            except Exception:
                pass


def stats_tile_rows(dim):
    """Rows per tile of the statistics kernel for feature dimension ``dim`` (tiles start at utterance-relative multiples)."""
    _check_dim(dim)
    r = C.c_int32()
    _capi.check(_capi.lib().pk_stats_tile_rows(int(dim), C.byref(r)))
    return r.value


def _check_dim(dim):
    if isinstance(dim, bool) or int(dim) != dim or dim < 1:
        raise ValueError(f"the feature dimension must be a positive integer, got {dim!r}")
    if dim > _capi.PK_STATS_MAX_DIM:
        raise NotImplementedError(f"feature dimension {dim}; the engine's envelope is 1 ... {_capi.PK_STATS_MAX_DIM}")


class FeatureStats:
    """Streaming mean / variance of feature matrices on the engine, with ``StandardScaler.partial_fit``'s attribute names.

    The state is a row count n, a shift K (float32, fixed once: ``shift=`` or the first row ever seen) and the float64 sums
    S1 = sum (x - K), S2 = sum (x - K)^2, accumulated in the fixed order csrc/pk_stats.h states: a corpus gives the same
    state bytes as one ragged batch, utterance by utterance or in any split into calls at utterance boundaries.  Inputs are
    (L, D) arrays or tensors ((L,) for D = 1) on the host or the device, read as float32.  NaN and Inf propagate (scikit-learn
    skips NaN; features here are never NaN).  ``merge`` and a different utterance order agree within rounding only."""

    def __init__(self, dim, shift=None, device=None):
        _check_dim(dim)
        self.dim = int(dim)
        self._shift0 = None if shift is None else self._check_shift(shift)
        self._device = device
        self._eng = None
        self._scratch = None
        self._set_host(0, self._shift0, np.zeros(self.dim), np.zeros(self.dim))

    # -- state ----------------------------------------------------------------
    def _check_shift(self, shift):
        k = to_numpy_f32(shift).reshape(-1)
        if k.shape != (self.dim,):
            raise ValueError(f"the shift has {k.size} entries, the feature dimension is {self.dim}")
        return k.copy()

    def _set_host(self, n, shift, s1, s2):
        self._n, self._k = int(n), None if shift is None else np.ascontiguousarray(shift, np.float32)
        self._s1, self._s2 = np.ascontiguousarray(s1, np.float64).copy(), np.ascontiguousarray(s2, np.float64).copy()

    def _engine(self):
        """The device accumulator; until the first update the state lives on the host (merge, state_dict and the derived
        values need no device)."""
        if self._eng is None:
            self._eng = _StatsEngine(self.dim, self._device)
            self._push(self._n, self._k, self._s1, self._s2)
        else:
            self._eng.ctx.bind_stream()
        return self._eng

    def _push(self, n, shift, s1, s2):
        e = self._eng
        _capi.check(e.ctx.lib.pk_stats_set(e.h, int(n), None if shift is None else _capi.fptr(shift), _capi.fptr(s1), _capi.fptr(s2)))

    def _state(self):
        """(n, K or None, S1, S2) as host arrays (synchronises when the state is on the device)."""
        if self._eng is None:
            return self._n, self._k, self._s1, self._s2
        e = self._eng
        n, have = C.c_int64(), C.c_int32()
        k, s1, s2 = np.empty(self.dim, np.float32), np.empty(self.dim, np.float64), np.empty(self.dim, np.float64)
        _capi.check(e.ctx.lib.pk_stats_get(e.h, C.byref(n), C.byref(have), _capi.fptr(k), _capi.fptr(s1), _capi.fptr(s2)))
        return n.value, (k if have.value else None), s1, s2

    def _load(self, n, shift, s1, s2):
        if self._eng is None:
            self._set_host(n, shift, s1, s2)
        else:
            self._push(n, None if shift is None else np.ascontiguousarray(shift, np.float32),
                       np.ascontiguousarray(s1, np.float64), np.ascontiguousarray(s2, np.float64))

    def reset(self):
        self._load(0, self._shift0, np.zeros(self.dim), np.zeros(self.dim))
        return self

    def state_dict(self):
        n, k, s1, s2 = self._state()
        return {"dim": self.dim, "n": int(n), "shift": None if k is None else k.copy(), "s1": s1.copy(), "s2": s2.copy()}

    def load_state_dict(self, state):
        if int(state["dim"]) != self.dim:
            raise ValueError(f"the state has feature dimension {state['dim']}, this accumulator {self.dim}")
        n, k = int(state["n"]), state["shift"]
        s1, s2 = (np.asarray(state[key], np.float64).reshape(-1) for key in ("s1", "s2"))
        if n < 0 or s1.shape != (self.dim,) or s2.shape != (self.dim,):
            raise ValueError("malformed FeatureStats state")
        if k is None and n > 0:
            raise ValueError("a state that has seen rows has a shift")
        self._load(n, None if k is None else self._check_shift(k), s1, s2)
        return self

    # -- input ----------------------------------------------------------------
    def _rows(self, x):
        """Shape checks on the host side of ``x`` (nothing is copied): -> number of rows."""
        shape = tuple(x.shape) if hasattr(x, "shape") else np.asarray(x).shape
        if not (len(shape) == 1 and self.dim == 1) and (len(shape) != 2 or shape[1] != self.dim):
            raise ValueError(f"expected a (L, {self.dim}) array" + (" or (L,)" if self.dim == 1 else "") + f", got shape {shape}")
        if shape[0] > _capi.PK_STATS_MAX_ROWS:
            raise NotImplementedError(f"an utterance of {shape[0]} rows; the engine's envelope is 2^31 - 1")
        return int(shape[0])

    def _check_list(self, xs):
        if isinstance(xs, (np.ndarray, torch.Tensor)):
            raise TypeError("a ragged batch is a list of (L, D) arrays; one array goes to partial_fit")
        xs = list(xs)
        return xs, np.asarray([self._rows(x) for x in xs], dtype=np.int64)

    def _pack(self, ctx, xs, lens):
        """The utterances as one (sum L, D) float32 device tensor."""
        parts = [ctx.to_device(x).reshape(-1, self.dim) for x, n in zip(xs, lens) if n]
        if not parts:
            return None
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)

    def _update(self, xs, lens):
        """Add the utterances to the state (the one method of this class that launches for fitting)."""
        e = self._engine()
        packed = self._pack(e.ctx, xs, lens)
        _capi.check(e.ctx.lib.pk_stats_update(e.h, None if packed is None else dptr(packed),
                                              lens.ctypes.data_as(C.POINTER(C.c_int64)), len(lens), None, 0))

    def _sums(self, xs, lens, shift):
        """Per-utterance (S1, S2) about ``shift`` as two (B, D) float64 host arrays; the state is not touched."""
        if self._scratch is None:
            self._scratch = _StatsEngine(self.dim, self._device)
        e = self._scratch
        e.ctx.bind_stream()
        _capi.check(e.ctx.lib.pk_stats_reset(e.h, _capi.fptr(np.ascontiguousarray(shift, np.float32))))
        packed = self._pack(e.ctx, xs, lens)
        out = torch.empty((len(lens), 2 * self.dim), dtype=torch.float64, device=e.ctx.device)
        _capi.check(e.ctx.lib.pk_stats_update(e.h, None if packed is None else dptr(packed),
                                              lens.ctypes.data_as(C.POINTER(C.c_int64)), len(lens), dptr(out),
                                              _capi.PK_STATS_MOMENTS_ONLY))
        u = out.cpu().numpy()
        return u[:, :self.dim].copy(), u[:, self.dim:].copy()

    @staticmethod
    def _first_row(xs, lens):
        for x, n in zip(xs, lens):
            if n:
                row = x[0]
                return to_numpy_f32(row).reshape(-1)
        return None

    # -- fitting --------------------------------------------------------------
    def partial_fit(self, x):
        """Add one (L, D) (or, for D = 1, (L,)) array or tensor."""
        return self.partial_fit_batch([x])

    def partial_fit_batch(self, xs):
        """Add a ragged list of utterances in one engine call; the same state bytes as adding them one by one."""
        xs, lens = self._check_list(xs)
        if len(xs):
            self._update(xs, lens)
        return self

    def fit(self, xs, groups=None):
        """``partial_fit_batch`` on a fresh accumulator -> self.  With ``groups`` (one hashable id per utterance): a dict
        {id: FeatureStats} of per-group statistics (per speaker, say), each the same bytes as fitting that group's
        utterances alone; this accumulator's own state is not touched."""
        xs, lens = self._check_list(xs)
        if groups is None:
            self.reset()
            if len(xs):
                self._update(xs, lens)
            return self
        groups = list(groups)
        if len(groups) != len(xs):
            raise ValueError(f"{len(groups)} group ids for {len(xs)} utterances")
        members = {}
        for i, g in enumerate(groups):
            members.setdefault(g, []).append(i)
        out = {}
        for g, idx in members.items():
            gx, gl = [xs[i] for i in idx], lens[idx]
            fs = type(self)(self.dim, shift=self._shift0, device=self._device)
            k = self._shift0 if self._shift0 is not None else self._first_row(gx, gl)
            if k is not None and gl.sum() > 0:
                u1, u2 = self._sums(gx, gl, k)
                s1, s2 = np.zeros(self.dim), np.zeros(self.dim)
                for a, b in zip(u1, u2):               # left to right, as the engine folds them
                    s1, s2 = s1 + a, s2 + b
                fs._load(int(gl.sum()), k, s1, s2)
            out[g] = fs
        return out

    def utterance_moments(self, xs):
        """Per-utterance (n, mean, M2): n (B,) int64, mean and M2 = sum (x - mean)^2 as (B, D) float64, from the utterances'
        own sums about this accumulator's shift (while that is open: about the first row of the list).  An utterance's
        values are the same bytes alone and in any batch for a given shift.  An empty utterance has mean = shift, M2 = 0.
        The state is not touched."""
        xs, lens = self._check_list(xs)
        k = self._state()[1]
        if k is None:
            k = self._first_row(xs, lens)
        if k is None:
            k = np.zeros(self.dim, np.float32)
        if len(xs) == 0:
            return lens, np.zeros((0, self.dim)), np.zeros((0, self.dim))
        u1, u2 = self._sums(xs, lens, k)
        nf = np.maximum(lens, 1).astype(np.float64)[:, None]
        mean = k.astype(np.float64)[None] + u1 / nf
        m2 = np.maximum(u2 - u1 * u1 / nf, 0.0)
        return lens, mean, m2

    def merge(self, other):
        """Add another accumulator's rows: its sums are re-shifted to this one's K on the host in float64 (within rounding
        of having seen the rows; not bit-reproducible across different K)."""
        if other.dim != self.dim:
            raise ValueError(f"cannot merge feature dimension {other.dim} into {self.dim}")
        n, k, s1, s2 = self._state()
        on, ok, o1, o2 = other._state()
        if on == 0:
            return self
        if k is None:
            self._load(on, ok, o1, o2)
            return self
        r1, r2 = reshift(on, ok, o1, o2, k)
        self._load(n + on, k, s1 + r1, s2 + r2)
        return self

    # -- derived --------------------------------------------------------------
    @property
    def n_samples_seen_(self):
        return int(self._state()[0])

    @property
    def shift_(self):
        k = self._state()[1]
        return None if k is None else k.copy()

    def _derived(self):
        n, k, s1, s2 = self._state()
        return derive_stats(n, k if k is not None else np.zeros(self.dim, np.float32), s1, s2)

    @property
    def mean_(self):
        return self._derived()[0]

    @property
    def var_(self):
        return self._derived()[1]

    @property
    def scale_(self):
        return self._derived()[2]

    def stats(self):
        """The (2, D) float32 array [mean, scale] the reference's compute_statistics.py saves."""
        mean, _, scale = self._derived()
        return np.stack([mean, scale]).astype(np.float32)

    def save(self, path):
        np.save(path, self.stats(), allow_pickle=False)

    def zscore(self):
        return ZScore.from_stats(self.stats())
