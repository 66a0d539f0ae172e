"""Dynamic time warping and its path statistics on the engine (csrc/dtw.hip) against the fp64 restatement
tests/dtw_ref.py, through the C ABI and through ``parakeet_amd.alignment`` / ``parakeet_amd.metrics``.

The local cost is separate IEEE float64 operations rounded to float32 once and the forward pass one float64 addition per cell,
so path, length and cost are compared with ``==`` (the cost bit for bit) in matrix mode and in feature mode; no tolerance is
involved.  The only tolerances of this file:
  * ``sum_sqrt``: the double-precision ``sqrt`` of HIP's math API table is listed with 1 ulp (the table tests/fp32_bounds.py
    and tests/test_mas_gpu.py already cite; the ROCm tree ships none), so every term is within 2^-52 relative and the sum of
    P non-negative terms adds P * 2^-53 relative: bound = (SQRT_ULP * 2^-52 + P * 2^-53) * sum_sqrt.
  * ``mel_cepstrum``: ``fp32_bounds.dot_bound`` for the exact-fp32 GEMM ``pk_op_matmul`` runs on.
  * the transposed wav: the frame-wise pitch picker's own measured error on the two signals plus 10 % (see the test).
First run on the MI355X (recorded in DESIGN.md 4.7b): SWEEP-RATIO sum_sqrt 0.0000, mel_cepstrum 0.0096 / 0.0326 / 0.0420 for
1 / 65 / 640 frames; picker RMS error 3.894e-4 and 2.131e-4 nats, tolerance 6.627e-4, |RMSE - ln(89 / 84)| = 3.2e-4."""
import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import dtw_ref as dr  # noqa: E402
import fp32_bounds as fb  # noqa: E402

pytestmark = pytest.mark.gpu

SQRT_ULP = 1                      # HIP math API table: sqrt (double), maximum ulp error (see the module docstring)
SENTINEL = -7
_LONG = (1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)
_SHORT = (1, 2, 64, 65)
SHAPES = sorted({(a, b) for a in _LONG for b in _SHORT} | {(b, a) for a in _LONG for b in _SHORT}) + [(1024, 1025)]
SMALL = [i for i, (N, M) in enumerate(SHAPES) if max(N, M) <= 65]
KINDS = ("random", "quantised", "constant")
_cache = {}


def _np(t):
    return t.as_subclass(torch.Tensor).detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _features(N, M, kind, seed, D=None):
    """x (N, D), y (M, D).  random: D = 3 normal features; quantised: D = 2 features in {0, 1}, so the costs are {0, 1, 2}-valued
    and ties are everywhere; constant: all costs equal."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        D = D or 3
        return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((M, D)).astype(np.float32)
    if kind == "quantised":
        return rng.integers(0, 2, size=(N, 2)).astype(np.float32), rng.integers(0, 2, size=(M, 2)).astype(np.float32)
    return np.full((N, 2), 0.75, np.float32), np.full((M, 2), 0.25, np.float32)


def _case(N, M, kind, seed, D=None):
    x, y = _features(N, M, kind, seed, D)
    c = dr.local_cost(x, y)
    return dict(x=x, y=y, c=c, ref=dr.dtw(c))


def _cases(kind):
    """The shapes' inputs and their reference results, computed once."""
    if kind not in _cache:
        _cache[kind] = [_case(N, M, kind, 100 * i + 11) for i, (N, M) in enumerate(SHAPES)]
        if kind == "quantised":
            assert all(set(np.unique(k["c"])) <= {0.0, 1.0, 2.0} for k in _cache[kind])
        if kind == "constant":
            assert all(np.all(k["c"] == k["c"][0, 0]) for k in _cache[kind])
    return _cache[kind]


def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _i64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int64)


def _call(mode, xbuf, ybuf, offs_x, offs_y, sx, sy, D, k0, k1, rows, cols, check=True):
    """pk_dtw_run on flat float32 host buffers -> (0, per-pair dicts) or (status code, message).  The path buffers start as
    SENTINEL; entries from P on must keep it."""
    from parakeet_amd import _capi
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    tx = ctx.to_device(np.ascontiguousarray(xbuf, dtype=np.float32).reshape(-1))
    ty = None if ybuf is None else ctx.to_device(np.ascontiguousarray(ybuf, dtype=np.float32).reshape(-1))
    rows, cols = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
    offs_x, offs_y = _i64(offs_x), _i64(offs_y)
    B = int(rows.size)
    cap = np.maximum(rows.astype(np.int64) + cols - 1, 0)
    po = np.concatenate(([0], np.cumsum(cap)))
    ix = torch.full((max(int(po[-1]), 1),), SENTINEL, dtype=torch.int32, device=ctx.device)
    iy = torch.full((max(int(po[-1]), 1),), SENTINEL, dtype=torch.int32, device=ctx.device)
    ln = torch.full((max(B, 1),), SENTINEL, dtype=torch.int32, device=ctx.device)
    cost = torch.full((max(B, 1),), -1.0, dtype=torch.float64, device=ctx.device)
    status = torch.full((max(B, 1),), SENTINEL, dtype=torch.int32, device=ctx.device)
    rc = ctx.lib.pk_dtw_run(ctx.handle, int(mode), dptr(tx), None if ty is None else dptr(ty), _ptr(offs_x, C.c_int64),
                            _ptr(offs_y, C.c_int64), int(sx), int(sy), int(D), int(k0), int(k1), _ptr(rows, C.c_int32),
                            _ptr(cols, C.c_int32), B, dptr(ix), dptr(iy), dptr(ln), dptr(cost), dptr(status))
    ctx.sync()
    ixh, iyh, lnh, ch, sh = _np(ix), _np(iy), _np(ln), _np(cost), _np(status)
    if rc != 0:
        assert np.all(ixh == SENTINEL) and np.all(iyh == SENTINEL) and np.all(lnh == SENTINEL) and np.all(sh == SENTINEL)
        if check:
            _capi.check(rc)
        return rc, ctx.lib.pk_last_error().decode()
    out = []
    for b in range(B):
        P = int(lnh[b])
        assert 1 <= P <= cap[b]
        a, c = ixh[po[b]:po[b + 1]], iyh[po[b]:po[b + 1]]
        assert np.all(a[P:] == SENTINEL) and np.all(c[P:] == SENTINEL), "entries from P on are never written"
        out.append(dict(ix=a[:P], iy=c[:P], length=P, cost=ch[b], status=int(sh[b])))
    return 0, out


def _pack(arrs, order, gap=3):
    """The arrays in ``order``, each at an offset of its own in one buffer whose every other entry is NaN."""
    offs, o = [], gap
    for i in order:
        offs.append(o)
        o += arrs[i].size + gap
    buf = np.full(o, np.nan, dtype=np.float32)
    for i, off in zip(order, offs):
        buf[off:off + arrs[i].size] = arrs[i].reshape(-1)
    return buf, offs


def _matrix(cases, order, **kw):
    buf, offs = _pack([k["c"] for k in cases], order)
    return _call(0, buf, None, offs, None, 0, 0, 0, 0, 0, [cases[i]["c"].shape[0] for i in order],
                 [cases[i]["c"].shape[1] for i in order], **kw)


def _feature(cases, order, k0=0, k1=None, **kw):
    bx, ox = _pack([k["x"] for k in cases], order)
    by, oy = _pack([k["y"] for k in cases], order, gap=5)
    D = cases[order[0]]["x"].shape[1]
    return _call(1, bx, by, ox, oy, 0, 0, D, k0, D if k1 is None else k1, [cases[i]["x"].shape[0] for i in order],
                 [cases[i]["y"].shape[0] for i in order], **kw)


def _same(got, want, what):
    assert got["status"] == 0 and got["length"] == want["length"], what
    assert np.array_equal(got["ix"], want["ix"]) and np.array_equal(got["iy"], want["iy"]), what
    assert np.float64(got["cost"]).view(np.int64) == np.float64(want["cost"]).view(np.int64), (what, got["cost"], want["cost"])


@pytest.mark.parametrize("kind", KINDS)
def test_exact_in_a_ragged_batch_in_two_orders(kind):
    cases = _cases(kind)
    order = list(range(len(SHAPES)))
    for od in (order, order[::-1]):
        for run, mode in ((_matrix, "matrix"), (_feature, "features")):
            _, got = run(cases, od)
            for k, i in enumerate(od):
                _same(got[k], cases[i]["ref"], (kind, mode, SHAPES[i]))
    if kind == "constant":
        for (N, M), k in zip(SHAPES, cases):
            assert k["ref"]["length"] == max(N, M)                # every tie went to the diagonal


def test_each_pair_alone_and_contiguous():
    cases = _cases("random")
    for i, k in enumerate(cases):
        N, M = SHAPES[i]
        _, got = _call(0, k["c"], None, None, None, 0, 0, 0, 0, 0, [N], [M])
        _same(got[0], k["ref"], ("matrix", SHAPES[i]))
        _, got = _call(1, k["x"], k["y"], None, None, 0, 0, 3, 0, 3, [N], [M])
        _same(got[0], k["ref"], ("features", SHAPES[i]))
    sub = SMALL[::3]
    _, got = _call(0, np.concatenate([cases[i]["c"].reshape(-1) for i in sub]), None, None, None, 0, 0, 0, 0, 0,
                   [SHAPES[i][0] for i in sub], [SHAPES[i][1] for i in sub])
    for k, i in enumerate(sub):
        _same(got[k], cases[i]["ref"], SHAPES[i])


@pytest.mark.parametrize("kind", ["random", "quantised"])
def test_padded_tensors_with_poisoned_padding(kind):
    from parakeet_amd.alignment import dtw, dtw_features
    cases = _cases(kind)
    D = cases[0]["x"].shape[1]
    # every shape, in four padded tensors by size class so that no tensor is large: (B, Nmax + 2, Mmax + 3) costs, NaN elsewhere
    groups = {}
    for i, (N, M) in enumerate(SHAPES):
        groups.setdefault((N > 65, M > 65), []).append(i)
    assert len(groups) == 4
    for idx in groups.values():
        Nm, Mm = max(SHAPES[i][0] for i in idx) + 2, max(SHAPES[i][1] for i in idx) + 3
        B = len(idx)
        pc = np.full((B, Nm, Mm), np.nan, dtype=np.float32)
        px, py = np.full((B, Nm, D), np.nan, dtype=np.float32), np.full((B, Mm, D), np.nan, dtype=np.float32)
        for k, i in enumerate(idx):
            N, M = SHAPES[i]
            pc[k, :N, :M], px[k, :N], py[k, :M] = cases[i]["c"], cases[i]["x"], cases[i]["y"]
        rows, cols = [SHAPES[i][0] for i in idx], [SHAPES[i][1] for i in idx]
        _, got = _call(0, pc, None, np.arange(B) * Nm * Mm, None, Mm, 0, 0, 0, 0, rows, cols)
        _, gotf = _call(1, px, py, np.arange(B) * Nm * D, np.arange(B) * Mm * D, D, D, D, 0, D, rows, cols)
        for k, i in enumerate(idx):
            _same(got[k], cases[i]["ref"], SHAPES[i])
            _same(gotf[k], cases[i]["ref"], SHAPES[i])
    Nm, Mm = max(SHAPES[i][0] for i in SMALL), max(SHAPES[i][1] for i in SMALL)
    pc = np.full((len(SMALL), Nm, Mm), np.nan, dtype=np.float32)
    px, py = np.full((len(SMALL), Nm, D), np.nan, dtype=np.float32), np.full((len(SMALL), Mm, D), np.nan, dtype=np.float32)
    for k, i in enumerate(SMALL):
        N, M = SHAPES[i]
        pc[k, :N, :M], px[k, :N], py[k, :M] = cases[i]["c"], cases[i]["x"], cases[i]["y"]
    rows, cols = [SHAPES[i][0] for i in SMALL], [SHAPES[i][1] for i in SMALL]
    # the same through the Python interface: padded device tensors, lists of host arrays, one pair
    a = dtw(torch.from_numpy(pc), rows, cols)
    b = dtw([cases[i]["c"] for i in SMALL])
    f = dtw_features(torch.from_numpy(px), torch.from_numpy(py), x_lens=rows, y_lens=cols)
    g = dtw_features([cases[i]["x"] for i in SMALL], [cases[i]["y"] for i in SMALL])
    for k, i in enumerate(SMALL):
        ref = cases[i]["ref"]
        for r in (a[k], b[k], f[k], g[k]):
            assert np.array_equal(_np(r.ix), ref["ix"]) and np.array_equal(_np(r.iy), ref["iy"])
            assert r.cost == ref["cost"] and r.length == ref["length"] and _np(r.ix).dtype == np.int32
    one = dtw(cases[SMALL[7]]["c"])
    assert np.array_equal(_np(one.ix), cases[SMALL[7]]["ref"]["ix"]) and isinstance(one.cost, float)


@pytest.mark.parametrize("kind", KINDS)
def test_the_largest_pair(kind):
    k = _case(4096, 4096, kind, 77, D=2)
    _, got = _call(1, k["x"], k["y"], None, None, 0, 0, 2, 0, 2, [4096], [4096])
    _same(got[0], k["ref"], ("features", kind))
    _, got = _call(0, k["c"], None, None, None, 0, 0, 0, 0, 0, [4096], [4096])
    _same(got[0], k["ref"], ("matrix", kind))


def test_both_decision_stores():
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    w = C.c_int32()
    assert ctx.lib.pk_dtw_lds_words(C.byref(w)) == 0
    lds = int(w.value)
    assert 1024 <= lds <= 40960
    shapes = [(1024, lds // 64), (1024, lds // 64 + 1), (64, lds // 64), (64, lds // 64 + 1), (1500, 70), (70, 1500)]
    assert [dr.decision_words(N, M) <= lds for N, M in shapes] == [True, False, True, False, True, False]
    cases = [_case(N, M, KINDS[k % 3], 900 + k, D=2) for k, (N, M) in enumerate(shapes)]
    for run in (_matrix, _feature):
        _, got = run(cases, list(range(len(cases))))
        for k in range(len(cases)):
            _same(got[k], cases[k]["ref"], shapes[k])
    for k in (1, 3, 5):                                           # the global store alone: the workspace starts at this pair
        _, one = _matrix(cases, [k])
        _same(one[0], cases[k]["ref"], shapes[k])
        _, one = _feature(cases, [k])
        _same(one[0], cases[k]["ref"], shapes[k])


def test_cost_workspace_cap_splits_the_batch():
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    cases = _cases("random")
    sub = [i for i in range(len(SHAPES)) if SHAPES[i][0] * SHAPES[i][1] <= 70000][::2]
    old = C.c_int64()
    assert ctx.lib.pk_dtw_cost_cap(0, C.byref(old)) == 0 and old.value == 256 << 20
    try:
        assert ctx.lib.pk_dtw_cost_cap(4 * 70000, None) == 0      # a few pairs per launch, some alone and above the cap
        ctx.prof_enable(True)
        ctx.prof_reset()
        _, got = _feature(cases, sub)
        launches = ctx.prof_dump()["dtw_cost"][0]
    finally:
        ctx.prof_enable(False)
        assert ctx.lib.pk_dtw_cost_cap(old.value, None) == 0
    assert launches > 3
    for k, i in enumerate(sub):
        _same(got[k], cases[i]["ref"], SHAPES[i])


# ------------------------------------------------------------------------------------------------ feature mode's local cost
def _fma_cost(x, y, k0, k1):
    """The variant a contracting compiler would compute: s = fma(d, d, s), one rounding per column (exact rationals)."""
    s = 0.0
    for k in range(k0, k1):
        d = float(x[k]) - float(y[k])
        s = float(Fraction(d) * Fraction(d) + Fraction(s))
    return np.float32(s)


def _descending_cost(x, y, k0, k1):
    s = 0.0
    for k in range(k1 - 1, k0 - 1, -1):
        d = float(x[k]) - float(y[k])
        s = s + d * d
    return np.float32(s)


def _hostile_features(N, M, D, seed):
    """Values over many orders of magnitude; from D = 13 on, rows 0 and 1 of x against row 0 of y are built so that the float64
    sum sits on a float32 rounding boundary: a fused multiply-add (row 0) or another order of the sum (row 1) moves the cost."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, D)) * 10.0 ** rng.integers(-3, 4, size=(N, D))).astype(np.float32)
    y = (rng.standard_normal((M, D)) * 10.0 ** rng.integers(-3, 4, size=(M, D))).astype(np.float32)
    if D >= 13:
        x[:2], y[0] = 0.0, 0.0
        x[0, 1:5] = [3 * 2.0 ** -27, 3 * 2.0 ** -27, 2.0 ** -12, 1.0]
        y[0, 4] = 2.0 ** -51
        x[1, 1:7] = [1.0, 2.0 ** -12, 2.0 ** -27, 2.0 ** -27, 2.0 ** -27, 2.0 ** -27]
    return x, y


@pytest.mark.parametrize("D", [1, 13, 14, 80, 128])
def test_feature_cost_is_the_definition(D):
    from parakeet_amd.alignment import dtw_features
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    N, M = 37, 45
    x, y = _hostile_features(N, M, D, 300 + D)
    for k0, k1 in ((0, D), (1, D), (5, 6)):
        if not 0 <= k0 < k1 <= D:
            continue
        want = dr.local_cost(x, y, k0, k1)
        assert np.isfinite(want).all()
        if D >= 13 and k1 - k0 > 1:                              # on the CPU: the input does tell the variants apart
            assert want[0, 0] == 1.0 and _fma_cost(x[0], y[0], k0, k1) != want[0, 0]
            assert want[1, 0] == 1.0 and _descending_cost(x[1], y[0], k0, k1) != want[1, 0]
        # a padded layout with NaN in the padding columns' place would be read if the range were not respected
        xp, yp = np.full((N, D + 3), np.nan, np.float32), np.full((M, D + 2), np.nan, np.float32)
        xp[:, :D], yp[:, :D] = x, y
        if k0 > 0:
            xp[:, :k0], yp[:, :k0] = np.nan, np.nan
        if k1 < D:
            xp[:, k1:], yp[:, k1:] = np.nan, np.nan
        out = ctx.empty((N * M,))
        rows, cols = np.array([N], np.int32), np.array([M], np.int32)
        zero = np.zeros(1, np.int64)
        tx, ty = ctx.to_device(xp), ctx.to_device(yp)
        assert ctx.lib.pk_dtw_cost(ctx.handle, dptr(tx), dptr(ty), _ptr(zero, C.c_int64), _ptr(zero, C.c_int64), D + 3, D + 2, D, k0,
                                   k1, _ptr(rows, C.c_int32), _ptr(cols, C.c_int32), 1, dptr(out)) == 0
        got = _np(out).reshape(N, M)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (D, k0, k1)
        _, run = _call(1, xp, yp, zero, zero, D + 3, D + 2, D, k0, k1, [N], [M])
        ref = dr.dtw(want)
        _same(run[0], ref, (D, k0, k1))
        p = dtw_features(x, y, (k0, k1))
        assert np.array_equal(_np(p.ix), ref["ix"]) and p.cost == ref["cost"]


def test_status():
    from parakeet_amd.alignment import dtw, dtw_features
    rng = np.random.default_rng(12)
    N, M = 70, 66
    c = rng.random((N, M)).astype(np.float32)
    ref = dr.dtw(c)
    for bad_value in (np.nan, np.inf):
        for cell in ((0, 0), (N - 1, M - 1), (40, 17)):
            bad = c.copy()
            bad[cell] = bad_value
            assert dr.dtw(bad)["status"] == 1
            cases = [dict(c=c), dict(c=bad), dict(c=c)]
            _, got = _matrix(cases, [0, 1, 2])
            assert [g["status"] for g in got] == [0, 1, 0]
            _same(got[0], ref, "clean")
            _same(got[2], ref, "clean")
            assert got[1]["ix"][0] == 0 and got[1]["iy"][0] == 0 and got[1]["ix"][-1] == N - 1 and got[1]["iy"][-1] == M - 1
            with pytest.raises(FloatingPointError, match=r"pair\(s\) \[1\]"):
                dtw([c, bad, c])
    x, y = rng.standard_normal((9, 4)).astype(np.float32), rng.standard_normal((7, 4)).astype(np.float32)
    xb = x.copy()
    xb[3, 2] = np.nan
    with pytest.raises(FloatingPointError, match=r"pair\(s\) \[0\]"):
        dtw_features([xb, x], [y, y])
    xb[3, 2] = 3e38                                              # the squared distance overflows float32: inf
    with pytest.raises(FloatingPointError, match=r"pair\(s\) \[1\]"):
        dtw_features([x, xb], [y, y], (2, 3))
    ok = dtw_features(xb, y, (0, 2))                             # the column is outside the range: never read
    assert np.array_equal(_np(ok.ix), dr.dtw_features(x, y, 0, 2)["ix"])


def test_envelope_and_argument_refusals_launch_nothing():
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    tiny = np.zeros(8, np.float32)
    ctx.sync()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        for mode in (0, 1):
            rc, msg = _call(mode, tiny, tiny, None, None, 0, 0, 2, 0, 2, [4097], [2], check=False)
            assert rc == -3 and "4097 rows" in msg and "4096" in msg
            rc, msg = _call(mode, tiny, tiny, None, None, 0, 0, 2, 0, 2, [2, 2], [2, 4097], check=False)
            assert rc == -3 and "pair 1 has 4097 columns" in msg
            rc, msg = _call(mode, tiny, tiny, None, None, 0, 0, 2, 0, 2, [2, 0], [2, 1], check=False)
            assert rc == -1 and "pair 1 is empty" in msg
            rc, msg = _call(mode, tiny, tiny, None, None, 0, 0, 2, 0, 2, [], [], check=False)
            assert rc == -1 and "batch size" in msg
            rc, msg = _call(mode, tiny, tiny, None, None, 3, 0, 2, 0, 2, [2], [2], check=False)
            assert rc == -1 and "stride" in msg
        rc, msg = _call(1, tiny, tiny, None, None, 0, 0, 129, 0, 2, [2], [2], check=False)
        assert rc == -3 and "129" in msg and "128" in msg
        for k0, k1 in ((2, 2), (-1, 2), (0, 3), (1, 0)):
            rc, msg = _call(1, tiny, tiny, None, None, 0, 0, 2, k0, k1, [2], [2], check=False)
            assert rc == -1 and "column range" in msg
        rc, msg = _call(1, tiny, None, None, None, 0, 0, 2, 0, 2, [2], [2], check=False)
        assert rc == -1 and "NULL" in msg
        rc, msg = _call(2, tiny, tiny, None, None, 0, 0, 2, 0, 2, [2], [2], check=False)
        assert rc == -1 and "mode" in msg
        rc, msg = _call(0, tiny, None, [0], None, 1, 0, 0, 0, 0, [2], [2], check=False)
        assert rc == -1 and "row stride 1 below its 2 columns" in msg
        assert all(n == 0 for k, (n, _) in ctx.prof_dump().items() if k.startswith("dtw"))
        c = np.random.default_rng(1).random((9, 4)).astype(np.float32)
        _, got = _call(0, c, None, None, None, 0, 0, 0, 0, 0, [9], [4])
        _same(got[0], dr.dtw(c), "after the refusals")
        assert ctx.prof_dump()["dtw"][0] == 1
    finally:
        ctx.prof_enable(False)


# ----------------------------------------------------------------------------------------------------------- path statistics
def test_path_stats():
    from parakeet_amd.alignment import dtw_features, path_stats
    rng = np.random.default_rng(21)
    shapes = [(1, 1, 1), (300, 280, 13), (64, 700, 5), (1025, 65, 14), (17, 16, 128)]
    xs = [rng.standard_normal((N, D)).astype(np.float32) for N, M, D in shapes]
    ys = [rng.standard_normal((M, D)).astype(np.float32) for N, M, D in shapes]
    worst = 0.0
    for (N, M, D), x, y in zip(shapes, xs, ys):
        cols = (1, D) if D > 1 else (0, 1)
        path = dtw_features(x, y, cols)
        ref = dr.dtw_features(x, y, *cols)
        assert np.array_equal(_np(path.ix), ref["ix"])
        mx, my = rng.random(N) < 0.7, rng.random(M) < 0.7
        for masks in ((None, None), (mx, my), (mx, None)):
            got = path_stats(path, x, y, cols, *masks)
            want = dr.path_stats(ref["ix"], ref["iy"], x, y, *cols, *masks)
            assert got.sum_sq == want["sum_sq"] and got.length == ref["length"], (N, M, D)
            assert [got.n11, got.n10, got.n01, got.n00] == want["counts"].tolist()
            bound = (SQRT_ULP * 2.0 ** -52 + ref["length"] * 2.0 ** -53) * want["sum_sqrt"]
            if want["sum_sqrt"] == 0.0:
                assert got.sum_sqrt == 0.0
            else:
                worst = max(worst, abs(got.sum_sqrt - want["sum_sqrt"]) / bound)
    print(f"SWEEP-RATIO dtw path_stats sum_sqrt against fp64, bound ({SQRT_ULP} ulp + P / 2) * 2^-52: {worst:.4f}")
    assert worst <= 1.0
    # a batch (the buffers of one dtw call in place), the same pairs reversed (repacked), (ix, iy) arrays: the same bits
    x13 = [rng.standard_normal((n, 13)).astype(np.float32) for n in (50, 3, 200)]
    y13 = [rng.standard_normal((m, 13)).astype(np.float32) for m in (40, 9, 210)]
    paths = dtw_features(x13, y13, (1, 13))
    a = path_stats(paths, x13, y13, (1, 13))
    b = path_stats(paths[::-1], x13[::-1], y13[::-1], (1, 13))
    c = path_stats([(_np(p.ix), _np(p.iy)) for p in paths], x13, y13, (1, 13))
    for k in range(3):
        want = dr.path_stats(_np(paths[k].ix), _np(paths[k].iy), x13[k], y13[k], 1, 13)
        assert a[k].sum_sq == want["sum_sq"] and a[k] == b[2 - k] == c[k] == path_stats(paths[k], x13[k], y13[k], (1, 13))
    with pytest.raises(ValueError, match="leave their pair"):
        path_stats([(np.array([0, 60]), np.array([0, 39]))], x13[:1], y13[:1])
    with pytest.raises(ValueError, match="path 0 is one of a 50 x 40 pair"):
        path_stats(paths[:1], x13[1:2], y13[1:2])


# ------------------------------------------------------------------------------------------------------------ the metrics
@pytest.mark.parametrize("frames", [1, 65, 640])
def test_mel_cepstrum_against_fp64(frames):
    from parakeet_amd import metrics as mt
    rng = np.random.default_rng(frames)
    logmel = (rng.standard_normal((frames, 80)) * 1.5 - 3.0).astype(np.float32)
    got = _np(mt.mel_cepstrum(logmel, 13, 10.0))
    w64 = math.log(10.0) * mt.dct_matrix(80, 13)
    want = logmel.astype(np.float64) @ w64
    bound = fb.dot_bound(np.abs(logmel).astype(np.float64) @ np.abs(w64), 80)
    r = fb.ratio(got, want, bound)
    print(f"SWEEP-RATIO mel_cepstrum ({frames}, 80) against the fp64 product, dot_bound K = 80: {r:.4f}")
    assert got.shape == (frames, 14) and r <= 1.0
    two = mt.mel_cepstrum([logmel, logmel[: max(1, frames // 2)]], 13, 10.0)
    assert np.array_equal(_np(two[0]), got) and np.array_equal(_np(two[1]), got[: max(1, frames // 2)])
    nat = _np(mt.mel_cepstrum((logmel * np.float32(math.log(10.0))), 13, math.e))
    assert fb.ratio(nat, want, 2 * bound + 2 * fb.U * np.abs(want)) <= 1.0


SR, HOP = 24000, 300


def _harmonic(f0_frames, hop=HOP, sr=SR):
    """A harmonic signal whose f0 follows ``f0_frames`` (Hz per hop, linearly interpolated; all voiced) and whose harmonics'
    weights drift, so that the spectral envelope gives the warping something to align on.  -> (wav, f0 per sample)."""
    n = (len(f0_frames) - 1) * hop
    t = np.arange(n) / hop
    f0 = np.interp(t, np.arange(len(f0_frames)), f0_frames)
    phase = 2 * np.pi * np.cumsum(f0) / sr
    wav = sum(a * (1.0 + 0.8 * np.sin(2 * np.pi * t / period + h)) * np.sin(h * phase)
              for h, a, period in ((1, 0.4, 23.0), (2, 0.2, 17.0), (3, 0.1, 13.0), (4, 0.05, 29.0)))
    return wav.astype(np.float32), f0


def _signals():
    if "signals" not in _cache:
        from parakeet_amd import audio
        frames = 60
        contour = 150.0 + 1.5 * np.sin(np.linspace(0, 3.0, frames))
        wav, f0 = _harmonic(contour)
        # the copy transposed by one semitone: played back 2^(1/12) faster (resampled to the rate sr / 2^(1/12), read at sr)
        up, down = 89, 84                                        # 89 / 84 = 1.05952 against 2^(1/12) = 1.05946
        tr = _np(audio.resample(wav, up * 100, down * 100)).astype(np.float32)
        _cache["signals"] = dict(wav=wav, f0=f0, tr=tr, ratio=up / down)
    return _cache["signals"]


def _pitch_error(pitch, wav, f0_true, scale, hop=HOP):
    """RMS error in nats of the frame-wise picker on a signal whose true contour is known: frame t is centred on sample t * hop
    of the signal; the transposed copy's sample n is the original's sample n * scale."""
    f = _np(pitch.track([wav])[0][0]).astype(np.float64)
    t = np.arange(len(f)) * hop * scale
    keep = (f > 0) & (t <= len(f0_true) - 1) & (np.arange(len(f)) >= 2) & (np.arange(len(f)) < len(f) - 2)
    true = np.interp(t[keep], np.arange(len(f0_true)), f0_true) * scale
    return float(np.sqrt(np.mean((np.log(f[keep]) - np.log(true)) ** 2))), f


def test_mcd_of_a_stretched_copy_is_zero_with_the_known_path():
    from parakeet_amd import audio, metrics as mt
    s = _signals()
    mel = audio.LogMelFBank(sr=SR, hop_length=HOP)
    ref = _np(mel.get_log_mel_fbank(s["wav"]))
    N = ref.shape[0]
    keep = np.concatenate(([True], np.any(ref[1:] != ref[:-1], axis=1)))      # pairwise distinct neighbours
    assert keep.all()
    d = np.random.default_rng(3).integers(1, 4, size=N)
    syn = np.repeat(ref, d, axis=0)
    out, path = mt.mcd_batch(ref, syn, return_paths=True)
    assert out["mcd"] == 0.0 and out["rows"] == N and out["cols"] == len(syn) == out["length"]
    assert out["length_ratio"] == len(syn) / N
    assert np.array_equal(_np(path.ix), np.repeat(np.arange(N), d)) and np.array_equal(_np(path.iy), np.arange(len(syn)))
    both = mt.mcd_batch([ref, ref[:20]], [syn, ref[5:40]])
    assert both[0] == out and both[1]["mcd"] > 0.0 and both[1]["rows"] == 20 and both[1]["cols"] == 35
    f0 = (100.0 + np.arange(N)).astype(np.float32)
    f0[::7] = 0.0
    r = mt.f0_batch(path, f0, np.repeat(f0, d) * np.float32(2.0 ** (1.0 / 12.0)))
    P, nv = len(syn), int((np.repeat(f0, d) > 0).sum())
    assert r["voiced_both"] == nv and r["vuv_error"] == 0.0
    assert abs(r["f0_rmse_cents"] - 100.0) <= 1200.0 / math.log(2.0) * 4 * 2.0 ** -24 * math.log(300.0)
    none = mt.f0_batch(path, np.zeros(N, np.float32), np.repeat(f0, d))
    assert math.isnan(none["f0_rmse"]) and none["vuv_error"] == nv / P and none["voiced_both"] == 0


def test_score_batch_on_a_transposed_copy_and_the_example(tmp_path, capsys):
    from parakeet_amd import audio, metrics as mt
    import score_synthesis as ex
    s = _signals()
    pitch = audio.Pitch(sr=SR, hop_length=HOP, f0min=80, f0max=400)
    mel = audio.LogMelFBank(sr=SR, hop_length=HOP)
    e_ref, _ = _pitch_error(pitch, s["wav"], s["f0"], 1.0)
    e_tr, _ = _pitch_error(pitch, s["tr"], s["f0"], s["ratio"])
    tol = 1.1 * (e_ref + e_tr)
    out = mt.score_batch([s["wav"], s["wav"]], [s["tr"], s["wav"]], SR, mel=mel, pitch=pitch)
    want = math.log(s["ratio"])
    accuracy = (f"PITCH-ACCURACY frame-wise picker RMS error [nats]: original {e_ref:.3e}, transposed {e_tr:.3e}; "
                f"log-F0 RMSE of the pair {out[0]['f0_rmse']:.6f} against ln(89 / 84) = {want:.6f}, tolerance {tol:.3e}")
    print(accuracy)
    assert abs(out[0]["f0_rmse"] - want) <= tol
    assert abs(out[0]["f0_rmse_cents"] - out[0]["f0_rmse"] * 1200 / math.log(2)) < 1e-9 and out[0]["mcd"] > 0.0
    assert out[0]["cols"] < out[0]["rows"] and out[0]["voiced_both"] > 40 and out[0]["vuv_error"] <= 0.1
    assert out[1]["mcd"] == 0.0 and out[1]["f0_rmse"] == 0.0 and out[1]["length"] == out[1]["rows"] == out[1]["cols"]
    # the example: wavs paired by name (the generated one at another rate), then log-mels from .npy
    for d in ("ref", "gen", "refmel", "genmel"):
        os.makedirs(tmp_path / d)
    audio.write_wav(str(tmp_path / "ref" / "a.wav"), s["wav"], SR, subtype="FLOAT")
    audio.write_wav(str(tmp_path / "ref" / "b.wav"), s["wav"], SR, subtype="FLOAT")
    audio.write_wav(str(tmp_path / "gen" / "a.wav"), s["tr"], SR, subtype="FLOAT")
    audio.write_wav(str(tmp_path / "gen" / "b.wav"), s["wav"], SR, subtype="FLOAT")
    audio.write_wav(str(tmp_path / "gen" / "unpaired.wav"), s["wav"], SR, subtype="FLOAT")
    capsys.readouterr()
    rows = ex.main(["--gen-dir", str(tmp_path / "gen"), "--ref-dir", str(tmp_path / "ref"), "--batch", "1", "--f0max", "400"])
    text = capsys.readouterr().out
    print(accuracy)                                              # (the captured line again, for the log)
    assert [r["utt_id"] for r in rows] == ["a", "b"] and "unpaired" not in text.split("\n")[1]
    assert rows[0]["mcd"] == out[0]["mcd"] and rows[0]["f0_rmse_cents"] == out[0]["f0_rmse_cents"] and rows[1]["mcd"] == 0.0
    lines = [ln for ln in text.splitlines() if ln and not ln.startswith("#")]
    assert lines[0].split("\t")[0] == "a" and lines[1].split("\t")[0] == "b" and lines[-1].split("\t")[0] == "MEAN"
    ref_mel = _np(mel.get_log_mel_fbank(s["wav"]))
    np.save(tmp_path / "refmel" / "a.npy", ref_mel)
    np.save(tmp_path / "genmel" / "a.npy", np.repeat(ref_mel, 2, axis=0))
    rows = ex.main(["--gen-mel-dir", str(tmp_path / "genmel"), "--ref-mel-dir", str(tmp_path / "refmel")])
    assert len(rows) == 1 and rows[0]["mcd"] == 0.0 and rows[0]["length_ratio"] == 2.0 and "f0_rmse" not in rows[0]
