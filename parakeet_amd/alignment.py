"""Durations from a teacher's attention: monotonic alignment search and focus rate on the HIP engine.

``monotonic_align`` is the best monotonic path through a score matrix (the dynamic programme of Glow-TTS's ``maximum_path``)
for ragged batches, ``durations_from_attention`` the same on ``log(max(A, eps))`` of attention maps with the post-step a
FastSpeech recipe needs, ``focus_rate`` / ``select_map`` FastSpeech's criterion for choosing a head, ``write_durations`` the
``utt|speaker|ph d ph d ...`` file examples/fastspeech2_features.py reads.  The definition is this project's own
(csrc/pk_align.h); these are a teacher's attention boundaries, NOT the Montreal Forced Aligner's forced alignment.  Maps that
are device tensors stay on the device: views of one packed tensor (what ``teacher_forced_batch`` returns) are addressed
in place.  Rows are decoder steps S, columns tokens T.

``dtw`` / ``dtw_features`` / ``path_stats`` (csrc/pk_dtw.h) are unconstrained dynamic time warping of two
sequences of different lengths and float64 sums along its path: what ``parakeet_amd.metrics`` takes mel-cepstral distortion
and log-F0 RMSE along.  That definition is this project's own too (squared Euclidean local cost, no band, no slope weights).

``edit_distance`` / ``edit_align`` / ``confusions`` (csrc/pk_edit.h) are the Levenshtein distance of token-id
sequences -- the recurrence of parakeet/utils/error_rate.py -- and the alignment it comes from (hits, substitutions, deletions,
insertions; this project's own tie rule): what ``parakeet_amd.utils.error_rate`` counts word and character errors with."""
import collections
import ctypes as C

import numpy as np
import torch

from . import _capi
from .runtime import Context, dptr, wrap

__all__ = ["monotonic_align", "durations_from_attention", "focus_rate", "select_map", "write_durations", "MAX_TOKENS",
           "MAX_ROWS", "dtw", "dtw_features", "path_stats", "DTWPath", "PathStats", "DTW_MAX_FRAMES", "DTW_MAX_DIM",
           "edit_distance", "edit_align", "confusions", "EditAlignment", "EditCounts", "Confusions", "EDIT_MAX_TOKENS",
           "EDIT_MAX_BATCH"]

MAX_TOKENS, MAX_ROWS = 1024, 16384        # csrc/pk_align.h: MAS_MAX_COLS, MAS_MAX_ROWS


def _is_map(x):
    return isinstance(x, (np.ndarray, torch.Tensor)) or (hasattr(x, "numpy") and hasattr(x, "shape"))


def _lengths(x, B, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().as_subclass(torch.Tensor).numpy()
    x = np.asarray(x).reshape(-1).astype(np.int64)
    if x.size != B:
        raise ValueError(f"{B} utterances, {x.size} {what}")
    return x


def _layout(x, rows, cols, lead):
    """The accepted forms -> (maps, rows, cols, G, lead_shape, single, padded).  ``lead``: the number of leading map
    dimensions an utterance may have (0 for the search, up to 2 for the focus rate).  maps: a list of per-utterance arrays /
    tensors, or the one padded tensor."""
    if (rows is None) != (cols is None):
        raise ValueError("rows and cols go together: the valid lengths of a padded (B, ..., Smax, Tmax) tensor")
    if rows is not None:
        if not _is_map(x) or not 3 <= len(x.shape) <= 3 + lead:
            raise ValueError("rows / cols describe one padded tensor of shape (B, Smax, Tmax)" +
                             (" or (B, ..., Smax, Tmax)" if lead else "") + f", got {type(x).__name__}"
                             + (f" of shape {tuple(x.shape)}" if _is_map(x) else ""))
        B = int(x.shape[0])
        if B == 0:
            raise ValueError("no utterances given")
        r, c = _lengths(rows, B, "row counts"), _lengths(cols, B, "column counts")
        if (r < 1).any() or (c < 1).any() or (r > x.shape[-2]).any() or (c > x.shape[-1]).any():
            raise ValueError(f"lengths {r.tolist()} x {c.tolist()} do not lie in 1 ... {int(x.shape[-2])} x {int(x.shape[-1])}")
        ls = tuple(int(v) for v in x.shape[1:-2])
        return x, r, c, int(np.prod(ls, dtype=np.int64)), ls, False, True
    single = _is_map(x)
    maps = [x] if single else list(x)
    if not maps:
        raise ValueError("no utterances given")
    ls = None
    for b, m in enumerate(maps):
        if not _is_map(m) or not 2 <= len(m.shape) <= 2 + lead:
            raise ValueError(f"utterance {b}: expected a map of shape " + ("(..., S, T)" if lead else "(S, T)") +
                             (f", got shape {tuple(m.shape)}" if _is_map(m) else f", got {type(m).__name__}"))
        if min(m.shape) < 1:
            raise ValueError(f"utterance {b} is empty: shape {tuple(m.shape)}")
        l = tuple(int(v) for v in m.shape[:-2])
        if ls is not None and l != ls:
            raise ValueError(f"utterance {b} has maps {l}, utterance 0 has {ls}")
        ls = l
    r = np.array([m.shape[-2] for m in maps], dtype=np.int64)
    c = np.array([m.shape[-1] for m in maps], dtype=np.int64)
    return maps, r, c, int(np.prod(ls, dtype=np.int64)), ls, single, False


def _check_envelope(r, c):
    for b in range(r.size):
        if c[b] > r[b]:
            raise ValueError(f"utterance {b} has more tokens ({int(c[b])}) than rows ({int(r[b])}): no monotonic path gives "
                             "every token a row")
    for b in range(r.size):
        if c[b] > MAX_TOKENS:
            raise NotImplementedError(f"utterance {b} has {int(c[b])} tokens; the engine's envelope is 1 ... {MAX_TOKENS}")
        if r[b] > MAX_ROWS:
            raise NotImplementedError(f"utterance {b} has {int(r[b])} rows; the engine's envelope is 1 ... {MAX_ROWS}")


def _device_ok(t, ctx):
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.device == ctx.device and t.dtype == torch.float32
            and t.is_contiguous())


def _place(ctx, maps, r, c, G, padded):
    """-> (keep, pointer, offs (B,) int64, map_stride, row_stride): where the engine finds the maps.  Nothing is copied when
    the maps are float32 views of one device tensor (or one padded device tensor); anything else is packed by one device
    concatenation (device tensors) or one upload (host arrays)."""
    B = r.size
    if padded:
        t = maps if _device_ok(maps, ctx) else ctx.to_device(maps)
        Sm, Tm = int(t.shape[-2]), int(t.shape[-1])
        return t, dptr(t), np.arange(B, dtype=np.int64) * (G * Sm * Tm), Sm * Tm, Tm
    if all(_device_ok(m, ctx) for m in maps):
        ts = [m.as_subclass(torch.Tensor) for m in maps]
        if len({t.untyped_storage().data_ptr() for t in ts}) == 1:
            base = min(t.data_ptr() for t in ts)
            return ts, C.c_void_p(base), np.array([(t.data_ptr() - base) // 4 for t in ts], dtype=np.int64), 0, 0
        flat = torch.cat([t.reshape(-1) for t in ts])
    elif all(isinstance(m, torch.Tensor) and m.is_cuda for m in maps):
        flat = torch.cat([m.as_subclass(torch.Tensor).to(device=ctx.device, dtype=torch.float32).reshape(-1) for m in maps])
    else:
        host = [m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else (np.asarray(m.numpy()) if hasattr(m, "numpy")
                                                                             and not isinstance(m, np.ndarray) else m)
                for m in maps]
        flat = ctx.to_device(np.concatenate([np.asarray(h, dtype=np.float32).reshape(-1) for h in host]))
    offs = np.concatenate(([0], np.cumsum(G * r * c)[:-1])).astype(np.int64)
    return flat, dptr(flat), offs, 0, 0


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def _run(x, rows, cols, mode, eps, return_path, return_v):
    maps, r, c, _, _, single, padded = _layout(x, rows, cols, 0)
    _check_envelope(r, c)
    ctx = Context.get()
    keep, ptr, offs, _, row_stride = _place(ctx, maps, r, c, 1, padded)
    B = int(r.size)
    r32, c32 = _i32(r), _i32(c)
    dur = ctx.empty((int(c.sum()),), dtype=torch.int32)
    path = ctx.empty((int(r.sum()),), dtype=torch.int32) if return_path else None
    score = ctx.empty((B,), dtype=torch.float64)
    status = ctx.empty((B,), dtype=torch.int32)
    v = ctx.empty((int((r * c).sum()),)) if return_v else None
    _capi.check(ctx.lib.pk_mas_run(ctx.handle, ptr, _p(offs, C.c_int64), int(row_stride), _p(r32, C.c_int32), _p(c32, C.c_int32),
                                   B, int(mode), float(eps), dptr(dur), None if path is None else dptr(path), dptr(score),
                                   dptr(status), None if v is None else dptr(v)))
    st = status.cpu().numpy()
    del keep
    if st.any():
        bad = [int(b) for b in np.flatnonzero(st)]
        raise FloatingPointError(f"monotonic alignment: utterance(s) {bad} hold a score that is not finite in a reachable cell "
                                 "(column <= row)")
    d, sc = dur.cpu().numpy(), score.cpu().numpy()
    p = path.cpu().numpy() if return_path else None
    co, ro, vo = np.concatenate(([0], np.cumsum(c))), np.concatenate(([0], np.cumsum(r))), np.concatenate(([0], np.cumsum(r * c)))
    durs = [d[co[b]:co[b + 1]].copy() for b in range(B)]
    paths = [p[ro[b]:ro[b + 1]].copy() for b in range(B)] if return_path else None
    vs = [wrap(v[vo[b]:vo[b + 1]].view(int(r[b]), int(c[b]))) for b in range(B)] if return_v else None
    return single, durs, sc, paths, vs


def monotonic_align(scores, rows=None, cols=None, *, return_path=False):
    """Monotonic alignment search (``pk_mas_run``, scores mode).  ``scores``: one (S, T) map, a list of (S_b, T_b) maps, or a
    padded (B, Smax, Tmax) tensor with ``rows`` / ``cols`` (B,), the valid lengths; float32, numpy or tensors on any device.
    Returns ``(durations, score)`` or, with ``return_path``, ``(durations, score, path)``: per utterance the int32 numpy
    durations (T_b,) (each >= 1, sum S_b), the float64 path score Q(S - 1, T - 1) and the int32 numpy path (S_b,) -- lists
    (and a (B,) float64 array) for a list or a padded tensor, the bare items for one 2-D map.  ValueError names the utterance
    with more tokens than rows; NotImplementedError outside 1 <= T <= 1024, S <= 16384; FloatingPointError when a score in a
    reachable cell (column <= row) is not finite."""
    single, durs, sc, paths, _ = _run(scores, rows, cols, 0, 0.0, return_path, False)
    out = (durs[0], float(sc[0])) if single else (durs, sc)
    if return_path:
        out += (paths[0] if single else paths,)
    return out


def durations_from_attention(att, rows=None, cols=None, *, eps=1e-8, reduction_factor=1, merge_last=False,
                             return_scores=False):
    """Durations of attention maps (``pk_mas_run``, attention mode: the search on ``logf(max(A, eps))`` formed on the device).
    ``att`` as ``scores`` of ``monotonic_align``.  ``merge_last``: the last column's rows go to the column before it and the
    column is dropped (the <eos> column of a TransformerTTS map; needs T >= 2); ``reduction_factor`` multiplies the counts (a
    TransformerTTS decoder step is r frames).  Returns ``(durations, score)`` and, with ``return_scores``, the (S_b, T_b) device
    tensors of the scores the search used as a third item."""
    r = int(reduction_factor)
    if r < 1:
        raise ValueError(f"reduction_factor {reduction_factor} must be a positive integer")
    if not (float(eps) > 0.0 and np.isfinite(np.float32(eps)) and np.float32(eps) > 0):
        raise ValueError(f"eps {eps} must be a positive float32 number")
    if merge_last:
        c = _layout(att, rows, cols, 0)[2]
        if (c < 2).any():
            raise ValueError(f"merge_last needs at least two columns; utterance {int(np.flatnonzero(c < 2)[0])} has one")
    single, durs, sc, _, vs = _run(att, rows, cols, 1, eps, False, return_scores)
    durs = [_post(d, r, merge_last) for d in durs]
    out = (durs[0], float(sc[0])) if single else (durs, sc)
    if return_scores:
        out += (vs[0] if single else vs,)
    return out


def _post(d, r, merge_last):
    if merge_last:
        d = d.copy()
        d[-2] += d[-1]
        d = d[:-1]
    return (d * np.int32(r)).astype(np.int32)


def focus_rate(att, rows=None, cols=None):
    """FastSpeech's focus rate F = (1 / S) sum_s max_t A[s, t] of every map (``pk_focus_rate_run``).  ``att``: one utterance's
    maps (S, T), (G, S, T) or (layers, heads, S, T); a list of such (the same leading shape for all); or a padded
    (B, ..., Smax, Tmax) tensor with ``rows`` / ``cols``.  Returns float64 numpy of the leading shape per utterance (a list for
    a list or a padded tensor)."""
    maps, r, c, G, ls, single, padded = _layout(att, rows, cols, 2)
    ctx = Context.get()
    keep, ptr, offs, map_stride, row_stride = _place(ctx, maps, r, c, G, padded)
    B = int(r.size)
    out = ctx.empty((B * G,), dtype=torch.float64)
    g32, r32, c32 = np.full(B, G, dtype=np.int32), _i32(r), _i32(c)
    _capi.check(ctx.lib.pk_focus_rate_run(ctx.handle, ptr, _p(offs, C.c_int64), int(map_stride), int(row_stride),
                                          _p(g32, C.c_int32), _p(r32, C.c_int32), _p(c32, C.c_int32), B, dptr(out)))
    f = out.cpu().numpy().reshape((B,) + ls)
    del keep
    return f[0] if single else [f[b] for b in range(B)]


def select_map(att, rows=None, cols=None):
    """The index of the map with the largest focus rate per utterance (the first of equal ones): a tuple over the leading
    dimensions, ``(layer, head)`` for TransformerTTS's (dlayers, aheads, S, T + 1) maps."""
    f = focus_rate(att, rows, cols)
    pick = lambda a: tuple(int(i) for i in np.unravel_index(int(np.argmax(a)), a.shape))  # noqa: E731
    return [pick(a) for a in f] if isinstance(f, list) else pick(np.asarray(f))


def write_durations(path, utt_ids, speakers, phones, durations):
    """One ``utt|speaker|ph d ph d ...`` line per utterance (d in frames), the file ``read_durations`` of
    examples/fastspeech2_features.py reads.  ``speakers``: one name per utterance, or one name for all."""
    utt_ids = [str(u) for u in utt_ids]
    if isinstance(speakers, str):
        speakers = [speakers] * len(utt_ids)
    if not (len(utt_ids) == len(speakers) == len(phones) == len(durations)):
        raise ValueError(f"{len(utt_ids)} utterances, {len(speakers)} speakers, {len(phones)} phone lists, {len(durations)} duration lists")
    lines = []
    for u, spk, ph, d in zip(utt_ids, speakers, phones, durations):
        ph, d = [str(p) for p in ph], [int(v) for v in np.asarray(d).reshape(-1)]
        if len(ph) != len(d):
            raise ValueError(f"{u}: {len(ph)} phones, {len(d)} durations")
        if not ph:
            raise ValueError(f"{u}: no phones")
        for s in [u, str(spk)] + ph:
            if "|" in s or any(ch.isspace() for ch in s) or not s:
                raise ValueError(f"{u}: {s!r} cannot be written: names hold no '|' and no white space")
        if min(d) < 0:
            raise ValueError(f"{u}: a negative duration")
        lines.append(f"{u}|{spk}|" + " ".join(f"{p} {v}" for p, v in zip(ph, d)))
    with open(path, "wt", encoding="utf-8") as f:
        f.write("".join(line + "\n" for line in lines))


# --------------------------------------------------------------------------------------------- dynamic time warping (4.7b)
DTW_MAX_FRAMES, DTW_MAX_DIM = 4096, 128    # csrc/pk_dtw.h: DTW_MAX_ROWS / DTW_MAX_COLS, DTW_MAX_DIM

PathStats = collections.namedtuple("PathStats", "sum_sq sum_sqrt n11 n10 n01 n00 length")


class DTWPath:
    """One pair's warping path: ``ix``, ``iy`` int32 device tensors of ``length`` entries (forward, from (0, 0) to
    (rows - 1, cols - 1)), ``cost`` = Q(rows - 1, cols - 1) as a float."""
    __slots__ = ("ix", "iy", "cost", "length", "rows", "cols", "_batch", "_index")

    def __init__(self, ix, iy, cost, length, rows, cols, batch=None, index=0):
        self.ix, self.iy, self.cost, self.length, self.rows, self.cols = ix, iy, float(cost), int(length), int(rows), int(cols)
        self._batch, self._index = batch, index

    def __repr__(self):
        return f"DTWPath({self.rows} x {self.cols}, length={self.length}, cost={self.cost!r})"


def _dtw_envelope(r, c):
    for b in range(r.size):
        if r[b] > DTW_MAX_FRAMES:
            raise NotImplementedError(f"pair {b} has {int(r[b])} rows; the engine's envelope is 1 ... {DTW_MAX_FRAMES}")
        if c[b] > DTW_MAX_FRAMES:
            raise NotImplementedError(f"pair {b} has {int(c[b])} columns; the engine's envelope is 1 ... {DTW_MAX_FRAMES}")


def _features(x, lens, what):
    """One (n, D) sequence, a list of such, or a padded (B, nmax, D) tensor with ``lens`` -> (seqs, n (B,), D, single, padded)."""
    if lens is not None:
        if not _is_map(x) or len(x.shape) != 3:
            raise ValueError(f"{what}: lengths describe one padded tensor of shape (B, nmax, D), got "
                             + (f"shape {tuple(x.shape)}" if _is_map(x) else type(x).__name__))
        B = int(x.shape[0])
        if B == 0:
            raise ValueError(f"{what}: no sequences given")
        n = _lengths(lens, B, f"{what} lengths")
        if (n < 1).any() or (n > x.shape[1]).any():
            raise ValueError(f"{what}: lengths {n.tolist()} do not lie in 1 ... {int(x.shape[1])}")
        return x, n, int(x.shape[2]), False, True
    single = _is_map(x)
    seqs = [x] if single else list(x)
    if not seqs:
        raise ValueError(f"{what}: no sequences given")
    for b, m in enumerate(seqs):
        if not _is_map(m) or len(m.shape) != 2:
            raise ValueError(f"{what} {b}: expected features of shape (frames, D)"
                             + (f", got shape {tuple(m.shape)}" if _is_map(m) else f", got {type(m).__name__}"))
        if min(m.shape) < 1:
            raise ValueError(f"{what} {b} is empty: shape {tuple(m.shape)}")
        if m.shape[1] != seqs[0].shape[1]:
            raise ValueError(f"{what} {b} has {int(m.shape[1])} feature columns, {what} 0 has {int(seqs[0].shape[1])}")
    return seqs, np.array([m.shape[0] for m in seqs], dtype=np.int64), int(seqs[0].shape[1]), single, False


def _columns(columns, D):
    if D > DTW_MAX_DIM:
        raise NotImplementedError(f"feature dimension {D}; the engine's envelope is 1 ... {DTW_MAX_DIM}")
    k0, k1 = (0, D) if columns is None else (int(columns[0]), int(columns[1]))
    if not 0 <= k0 < k1 <= D:
        raise ValueError(f"columns [{k0}, {k1}) do not lie in [0, {D})")
    return k0, k1


def _pair_features(x, y, x_lens, y_lens, columns):
    xs, n, D, single, xpad = _features(x, x_lens, "x")
    ys, m, Dy, ysingle, ypad = _features(y, y_lens, "y")
    if n.size != m.size or single != ysingle:
        raise ValueError(f"{n.size} sequences x, {m.size} sequences y")
    if D != Dy:
        raise ValueError(f"x has {D} feature columns, y has {Dy}")
    k0, k1 = _columns(columns, D)
    _dtw_envelope(n, m)
    ctx = Context.get()
    dd = np.full(n.size, D, dtype=np.int64)
    kx, px, ox, _, sx = _place(ctx, xs, n, dd, 1, xpad)
    ky, py, oy, _, sy = _place(ctx, ys, m, dd, 1, ypad)
    return ctx, (kx, ky), px, py, ox, oy, int(sx), int(sy), D, k0, k1, n, m, single


def _dtw_call(ctx, mode, px, py, ox, oy, sx, sy, D, k0, k1, r, c, single, keep):
    B = int(r.size)
    r32, c32 = _i32(r), _i32(c)
    cap = (r + c - 1).astype(np.int64)
    po = np.concatenate(([0], np.cumsum(cap)))
    ix = ctx.empty((int(po[-1]),), dtype=torch.int32)
    iy = ctx.empty((int(po[-1]),), dtype=torch.int32)
    ln = ctx.empty((B,), dtype=torch.int32)
    cost = ctx.empty((B,), dtype=torch.float64)
    status = ctx.empty((B,), dtype=torch.int32)
    _capi.check(ctx.lib.pk_dtw_run(ctx.handle, int(mode), px, py, _p(ox, C.c_int64), None if oy is None else _p(oy, C.c_int64),
                                   int(sx), int(sy), int(D), int(k0), int(k1), _p(r32, C.c_int32), _p(c32, C.c_int32), B,
                                   dptr(ix), dptr(iy), dptr(ln), dptr(cost), dptr(status)))
    st, P, q = status.cpu().numpy(), ln.cpu().numpy(), cost.cpu().numpy()
    del keep
    if st.any():
        raise FloatingPointError(f"dynamic time warping: pair(s) {[int(b) for b in np.flatnonzero(st)]} hold a local cost that "
                                 "is not finite")
    batch = (ix, iy, ln, r32, c32)
    out = [DTWPath(wrap(ix[po[b]:po[b] + P[b]]), wrap(iy[po[b]:po[b] + P[b]]), q[b], P[b], r[b], c[b], batch, b)
           for b in range(B)]
    return out[0] if single else out


def dtw(cost, rows=None, cols=None):
    """Dynamic time warping through given local costs (``pk_dtw_run``, matrix mode).  ``cost``: one (N, M) matrix, a list of
    (N_b, M_b) matrices, or a padded (B, Nmax, Mmax) tensor with ``rows`` / ``cols`` (B,), the valid lengths; float32, numpy
    or tensors on any device (device tensors stay there; views of one packed tensor are addressed in place).  Returns a
    ``DTWPath`` (``ix``, ``iy``, ``cost``, ``length``) per pair: a list for a list or a padded tensor, the bare item for one
    matrix.  NotImplementedError outside 1 <= N, M <= 4096; FloatingPointError naming the pairs with a cost that is not
    finite."""
    maps, r, c, _, _, single, padded = _layout(cost, rows, cols, 0)
    _dtw_envelope(r, c)
    ctx = Context.get()
    keep, ptr, offs, _, row_stride = _place(ctx, maps, r, c, 1, padded)
    return _dtw_call(ctx, 0, ptr, None, offs, None, row_stride, 0, 0, 0, 0, r, c, single, keep)


def dtw_features(x, y, columns=None, *, x_lens=None, y_lens=None):
    """Dynamic time warping of feature sequences (``pk_dtw_run``, feature mode): the local cost is the squared Euclidean
    distance over the feature columns ``columns = (k0, k1)`` (all by default), formed on the device in float64 and rounded to
    float32 once.  ``x`` / ``y``: one (N, D) / (M, D) sequence each, two lists of such, or padded (B, Nmax, D) / (B, Mmax, D)
    tensors with ``x_lens`` / ``y_lens``.  Returns as ``dtw``.  NotImplementedError outside 1 <= N, M <= 4096, D <= 128."""
    ctx, keep, px, py, ox, oy, sx, sy, D, k0, k1, n, m, single = _pair_features(x, y, x_lens, y_lens, columns)
    return _dtw_call(ctx, 1, px, py, ox, oy, sx, sy, D, k0, k1, n, m, single, keep)


def _pack_paths(ctx, paths, n, m):
    """-> (ix, iy, len) device buffers in pk_dtw_run's layout for pairs of n x m frames.  The buffers of one ``dtw`` call are
    used as they are."""
    B = n.size
    if len(paths) != B:
        raise ValueError(f"{len(paths)} paths, {B} pairs of sequences")
    for b, p in enumerate(paths):
        if isinstance(p, DTWPath) and (p.rows, p.cols) != (int(n[b]), int(m[b])):
            raise ValueError(f"path {b} is one of a {p.rows} x {p.cols} pair, the sequences have {int(n[b])} x {int(m[b])} frames")
    b0 = paths[0]._batch if isinstance(paths[0], DTWPath) else None
    if b0 is not None and b0[2].numel() == B and b0[0].device == ctx.device \
            and all(isinstance(p, DTWPath) and p._batch is b0 and p._index == b for b, p in enumerate(paths)):
        return b0[0], b0[1], b0[2]
    cap = (n + m - 1).astype(np.int64)
    po = np.concatenate(([0], np.cumsum(cap)))
    ix = torch.zeros((int(po[-1]),), dtype=torch.int32, device=ctx.device)
    iy = torch.zeros((int(po[-1]),), dtype=torch.int32, device=ctx.device)
    ln = np.zeros(B, dtype=np.int32)
    for b, p in enumerate(paths):
        a, c = (p.ix, p.iy) if isinstance(p, DTWPath) else p
        a, c = ctx.to_device(a, dtype=torch.int32).reshape(-1), ctx.to_device(c, dtype=torch.int32).reshape(-1)
        if a.numel() != c.numel() or not 1 <= a.numel() <= cap[b]:
            raise ValueError(f"path {b}: {a.numel()} and {c.numel()} entries for a pair of {int(n[b])} x {int(m[b])} frames")
        ix[po[b]:po[b] + a.numel()] = a
        iy[po[b]:po[b] + a.numel()] = c
        ln[b] = a.numel()
    return ix, iy, ctx.to_device(ln, dtype=torch.int32)


def _pack_masks(ctx, masks, lens, single, what):
    """Per-pair masks (or one padded (B, nmax) mask) -> one packed uint8 device tensor, sum of ``lens`` entries."""
    if masks is None:
        return None
    padded = not single and _is_map(masks)
    ms = [masks] if single else list(masks)
    if len(ms) != lens.size:
        raise ValueError(f"{len(ms)} {what} masks, {lens.size} pairs")
    out = []
    for b, mk in enumerate(ms):
        t = (mk.as_subclass(torch.Tensor) if isinstance(mk, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mk))).reshape(-1)
        if t.numel() < lens[b] or (not padded and t.numel() != lens[b]):
            raise ValueError(f"{what} mask {b} has {t.numel()} entries, the sequence {int(lens[b])} frames")
        out.append((t[:int(lens[b])] != 0).to(device=ctx.device, dtype=torch.uint8))
    return torch.cat(out).contiguous()


def path_stats(paths, x, y, columns=None, mask_x=None, mask_y=None, *, x_lens=None, y_lens=None):
    """Float64 sums along warping paths (``pk_dtw_path_stats``).  ``paths``: what ``dtw`` / ``dtw_features`` returned for
    these pairs (or ``(ix, iy)`` arrays); ``x`` / ``y`` and ``columns`` as for ``dtw_features``; ``mask_x`` / ``mask_y``: per
    pair a (N,) / (M,) mask (non-zero: set), or padded (B, Nmax) / (B, Mmax) masks.  With s_p the float64 squared distance of
    step p over the columns, returns per pair ``PathStats``: ``sum_sq`` = sum s_p and ``sum_sqrt`` = sum sqrt(s_p) over the
    steps whose two masks are set (all steps without masks), the counts ``n11, n10, n01, n00`` of the steps by (mask_x,
    mask_y), and the path's ``length``.  The sums are taken in a fixed order (csrc/pk_dtw.h): the same bits in any batch."""
    ctx, keep, px, py, ox, oy, sx, sy, D, k0, k1, n, m, single = _pair_features(x, y, x_lens, y_lens, columns)
    plist = [paths] if isinstance(paths, DTWPath) or (single and isinstance(paths, tuple)) else list(paths)
    ix, iy, ln = _pack_paths(ctx, plist, n, m)
    mx, my = _pack_masks(ctx, mask_x, n, single, "x"), _pack_masks(ctx, mask_y, m, single, "y")
    B = int(n.size)
    r32, c32 = _i32(n), _i32(m)
    sums = ctx.empty((B, 2), dtype=torch.float64)
    counts = ctx.empty((B, 4), dtype=torch.int64)
    status = ctx.empty((B,), dtype=torch.int32)
    _capi.check(ctx.lib.pk_dtw_path_stats(ctx.handle, dptr(ix), dptr(iy), dptr(ln), px, py, _p(ox, C.c_int64), _p(oy, C.c_int64),
                                          sx, sy, D, k0, k1, _p(r32, C.c_int32), _p(c32, C.c_int32), B,
                                          None if mx is None else dptr(mx), None if my is None else dptr(my), dptr(sums),
                                          dptr(counts), dptr(status)))
    st, s, cn, P = status.cpu().numpy(), sums.cpu().numpy(), counts.cpu().numpy(), ln.cpu().numpy()
    del keep
    if st.any():
        raise ValueError(f"path statistics: the path(s) of pair(s) {[int(b) for b in np.flatnonzero(st)]} leave their pair")
    out = [PathStats(float(s[b, 0]), float(s[b, 1]), int(cn[b, 0]), int(cn[b, 1]), int(cn[b, 2]), int(cn[b, 3]), int(P[b]))
           for b in range(B)]
    return out[0] if single else out


# ------------------------------------------------------------------------------------- edit distance and its alignment (4.7c)
EDIT_MAX_TOKENS, EDIT_MAX_BATCH = 4096, 65535    # csrc/pk_edit.h: EDIT_MAX_LEN; pairs in one call of pk_edit_run
HIT, SUBSTITUTION, DELETION, INSERTION = 0, 1, 2, 3

EditCounts = collections.namedtuple("EditCounts", "hits substitutions deletions insertions")
Confusions = collections.namedtuple("Confusions", "substitutions deletions insertions")


class EditAlignment:
    """One pair's alignment: ``ops`` a uint8 device tensor of ``length`` entries in forward order (0 hit, 1 substitution,
    2 deletion, 3 insertion), ``distance`` = substitutions + deletions + insertions, ``counts`` an ``EditCounts``,
    ``ref_len`` / ``hyp_len`` the pair's lengths."""
    __slots__ = ("ops", "distance", "counts", "length", "ref_len", "hyp_len")

    def __init__(self, ops, distance, counts, length, ref_len, hyp_len):
        self.ops, self.distance, self.counts = ops, int(distance), EditCounts(*(int(c) for c in counts))
        self.length, self.ref_len, self.hyp_len = int(length), int(ref_len), int(hyp_len)

    def index_pairs(self):
        """``(ref_index, hyp_index)``: int64 numpy arrays of ``length`` entries, the ids a step pairs; -1 at a gap (the ref
        index of an insertion, the hyp index of a deletion)."""
        ops = self.ops.as_subclass(torch.Tensor).cpu().numpy()
        ri, hi = np.cumsum(ops != INSERTION) - 1, np.cumsum(ops != DELETION) - 1
        return np.where(ops != INSERTION, ri, -1).astype(np.int64), np.where(ops != DELETION, hi, -1).astype(np.int64)

    def __repr__(self):
        return f"EditAlignment({self.ref_len} x {self.hyp_len}, distance={self.distance}, {self.counts})"


def _is_scalar(v):
    return isinstance(v, (int, float, np.number)) or (isinstance(v, (np.ndarray, torch.Tensor)) and v.ndim == 0)


def _id_seqs(ctx, x, lens, what):
    """One id sequence, a list of them, or a padded (B, Lmax) tensor with ``lens`` -> (keep, pointer, offs (B,) int64,
    n (B,) int64, single).  An int32 device tensor is addressed in place; anything else is packed by one upload."""
    if lens is not None:
        if not _is_map(x) or len(x.shape) != 2:
            raise ValueError(f"{what}: lengths describe one padded tensor of shape (B, Lmax), got "
                             + (f"shape {tuple(x.shape)}" if _is_map(x) else type(x).__name__))
        B, L = int(x.shape[0]), int(x.shape[1])
        if B == 0:
            raise ValueError(f"{what}: no sequences given")
        n = _lengths(lens, B, f"{what} lengths")
        if (n < 0).any() or (n > L).any():
            raise ValueError(f"{what}: lengths {n.tolist()} do not lie in 0 ... {L}")
        ok = isinstance(x, torch.Tensor) and x.is_cuda and x.device == ctx.device and x.dtype == torch.int32 and x.is_contiguous()
        t = x.as_subclass(torch.Tensor) if ok else ctx.to_device(x, dtype=torch.int32)
        if t.numel() == 0:
            t = ctx.to_device(np.zeros(1, np.int32), dtype=torch.int32)
        return t, dptr(t), np.arange(B, dtype=np.int64) * L, n, False
    single = (_is_map(x) and len(x.shape) == 1) or (isinstance(x, (list, tuple)) and all(_is_scalar(v) for v in x))
    seqs = [x] if single else list(x)
    if not seqs:
        raise ValueError(f"{what}: no sequences given")
    host = []
    for b, s in enumerate(seqs):
        if isinstance(s, torch.Tensor):
            s = s.detach().as_subclass(torch.Tensor).cpu().numpy()
        a = np.asarray(s)
        if a.ndim != 1 and a.size:
            raise ValueError(f"{what} {b}: expected a sequence of ids, got shape {tuple(a.shape)}")
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{what} {b}: ids are integers, got {a.dtype}")
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError(f"{what} {b}: ids are int32")
        host.append(a.reshape(-1).astype(np.int32))
    n = np.array([a.size for a in host], dtype=np.int64)
    flat = np.concatenate(host) if n.sum() else np.zeros(1, np.int32)
    t = ctx.to_device(flat, dtype=torch.int32)
    return t, dptr(t), np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.int64), n, single


def _edit_call(ref, hyp, ref_lens, hyp_lens, mode):
    ctx = Context.get()
    kr, pr, o_r, n, single = _id_seqs(ctx, ref, ref_lens, "ref")
    kh, ph, o_h, m, hsingle = _id_seqs(ctx, hyp, hyp_lens, "hyp")
    if n.size != m.size or single != hsingle:
        raise ValueError(f"{n.size} sequences ref, {m.size} sequences hyp")
    B = int(n.size)
    for b in range(B):
        if n[b] > EDIT_MAX_TOKENS or m[b] > EDIT_MAX_TOKENS:
            raise NotImplementedError(f"pair {b} has {int(n[b])} ref ids and {int(m[b])} hyp ids; the engine's envelope is "
                                      f"0 ... {EDIT_MAX_TOKENS}")
    if B > EDIT_MAX_BATCH:
        raise NotImplementedError(f"{B} pairs; the engine's envelope is {EDIT_MAX_BATCH} in a call")
    n32, m32 = _i32(n), _i32(m)
    dist = ctx.empty((B,), dtype=torch.int32)
    po = np.concatenate(([0], np.cumsum(n + m)))
    counts = ops = ln = None
    if mode == 1:
        counts, ln = ctx.empty((B, 4), dtype=torch.int32), ctx.empty((B,), dtype=torch.int32)
        ops = ctx.empty((max(int(po[-1]), 1),), dtype=torch.uint8)
    _capi.check(ctx.lib.pk_edit_run(ctx.handle, pr, ph, _p(o_r, C.c_int64), _p(o_h, C.c_int64), _p(n32, C.c_int32),
                                    _p(m32, C.c_int32), B, int(mode), dptr(dist), None if counts is None else dptr(counts),
                                    None if ops is None else dptr(ops), None if ln is None else dptr(ln)))
    d = dist.cpu().numpy()
    del kr, kh
    if mode == 0:
        return int(d[0]) if single else d.astype(np.int64)
    cn, P = counts.cpu().numpy(), ln.cpu().numpy()
    out = [EditAlignment(wrap(ops[po[b]:po[b] + P[b]]), d[b], cn[b], P[b], n[b], m[b]) for b in range(B)]
    return out[0] if single else out


def edit_distance(ref, hyp, ref_lens=None, hyp_lens=None):
    """The Levenshtein distance of token-id sequences (``pk_edit_run``, mode 0: no alignment is kept).  ``ref`` / ``hyp``: one
    sequence of int32 ids each (a 1-D array, tensor or list of ints), two lists of such, or padded (B, Lmax) tensors with
    ``ref_lens`` / ``hyp_lens`` (the padding is never read; int32 device tensors are addressed in place).  Empty sequences are
    valid.  Returns an int for one pair, a (B,) int64 numpy array otherwise.  NotImplementedError outside 0 <= length <= 4096,
    B <= 65535."""
    return _edit_call(ref, hyp, ref_lens, hyp_lens, 0)


def edit_align(ref, hyp, ref_lens=None, hyp_lens=None):
    """The distance and the alignment it comes from (``pk_edit_run``, mode 1), inputs as ``edit_distance``.  Returns an
    ``EditAlignment`` per pair (a list for lists or padded tensors).  Of several minimal edit scripts the one of csrc/pk_edit.h
    is returned: walking back from the ends, a hit on equal ids, else substitution before deletion before insertion."""
    return _edit_call(ref, hyp, ref_lens, hyp_lens, 1)


def confusions(alignments, refs, hyps):
    """Host-side tallies over alignments: ``Confusions(substitutions, deletions, insertions)``, three ``Counter`` s keyed by
    (ref token, hyp token), by the deleted ref token and by the inserted hyp token.  ``refs`` / ``hyps``: the token sequences
    the ids stood for (any hashable tokens), one per alignment."""
    if isinstance(alignments, EditAlignment):
        alignments, refs, hyps = [alignments], [refs], [hyps]
    if not (len(alignments) == len(refs) == len(hyps)):
        raise ValueError(f"{len(alignments)} alignments, {len(refs)} references, {len(hyps)} hypotheses")
    sub, dele, ins = collections.Counter(), collections.Counter(), collections.Counter()
    for b, (al, r, h) in enumerate(zip(alignments, refs, hyps)):
        if (al.ref_len, al.hyp_len) != (len(r), len(h)):
            raise ValueError(f"alignment {b} is one of a {al.ref_len} x {al.hyp_len} pair, the sequences have {len(r)} x {len(h)} tokens")
        ops = al.ops.as_subclass(torch.Tensor).cpu().numpy()
        ri, hi = al.index_pairs()
        for p in np.flatnonzero(ops != HIT):
            if ops[p] == SUBSTITUTION:
                sub[(r[ri[p]], h[hi[p]])] += 1
            elif ops[p] == DELETION:
                dele[r[ri[p]]] += 1
            else:
                ins[h[hi[p]]] += 1
    return Confusions(sub, dele, ins)
