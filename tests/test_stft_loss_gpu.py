"""Multi-resolution STFT loss on the engine (csrc/stft_dist.hip, parakeet_amd/stft_loss.py) against the fp64 restatement of
tests/stft_loss_ref.py under its derived bound and against the reference's own numbers (tests/golden/stft_loss.npz): the
magnitudes and the sums at every resolution of stft_loss_cases (all four residues of the hop modulo 4 and the recipe's
three), the Python surface, batch invariance bit for bit, exact scaling, and the refusals.  ``SWEEP-RATIO`` lines give
error / bound.

First hardware run (information only): magnitudes 0.2845 on the silent signal (one rounding of sqrtf(1e-7f) at a
bound of 2u) and 0.0033 - 0.063 elsewhere, sums <= 0.022, the golden's magnitudes 0.004 - 0.073, the default losses
0.171446 / 0.227884.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import fp32_bounds as fb
import stft_loss_cases as lc
import stft_loss_ref as lr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(GOLD, "stft_loss.npz")))


@functools.lru_cache(maxsize=None)
def _eng(rs):
    from parakeet_amd.stft_loss import _DistEngine
    return _DistEngine([r.n_fft for r in rs], [r.hop for r in rs], [r.win for r in rs], "hann")


@functools.lru_cache(maxsize=None)
def _case(r):
    xs, ys = lc.batch(r)
    return xs, ys, [lr.sums_with_bound(x, y, r) for x, y in zip(xs, ys)]


@pytest.mark.parametrize("r", lc.RESOLUTIONS, ids=lc.res_id)
def test_magnitudes_and_sums_match_the_restatement(r):
    xs, ys, per = _case(r)
    eng = _eng((r,))
    mx, my = eng.magnitude(0, xs), eng.magnitude(0, ys)
    got = eng.sums(xs, ys)
    assert got.shape == (3, 1, 3) and got.dtype == np.float64
    for b in range(3):
        s, bs, fx, fy = per[b]
        assert mx[b].shape == fx.X.shape == (lc.num_frames(r, len(xs[b])), 1 + r.n_fft // 2)
        qm = max(fb.ratio(_np(mx[b]), fx.X, fx.b_X), fb.ratio(_np(my[b]), fy.X, fy.b_X))
        qs = fb.ratio(got[b, 0], s, bs)
        print(f"SWEEP-RATIO stft_loss engine {lc.res_id(r)} b={b} magnitude {qm:.4f} sums {qs:.4f}")
        assert qm <= 1.0 and qs <= 1.0
    # the silent signal sits on the floor, exactly
    assert (_np(mx[1]) == np.sqrt(np.float32(1e-7))).all()


def test_all_resolutions_in_one_handle_and_host_io():
    """One handle with the seven resolutions gives, resolution by resolution, the bits of the single-resolution handles; so
    does the call with host pointers."""
    from parakeet_amd import _capi
    rs = tuple(lc.RESOLUTIONS)
    xs, ys = lc.batch(lc.RESOLUTIONS[6])                    # long enough for the reflect padding of every resolution
    eng = _eng(rs)
    got = eng.sums(xs, ys)
    for i, r in enumerate(rs):
        assert np.array_equal(got[:, i], _eng((r,)).sums(xs, ys)[:, 0]), lc.res_id(r)
    lens = np.array([len(x) for x in xs], np.int32)
    hx, hy = np.concatenate(xs), np.concatenate(ys)
    out = np.full((3, len(rs), 3), np.nan)
    _capi.check(eng.ctx.lib.pk_stftd_run(eng.h, _capi.fptr(hx), _capi.fptr(hy), lens.ctypes.data_as(C.POINTER(C.c_int32)), 3,
                                         out.ctypes.data_as(C.c_void_p), _capi.PK_HOST_IO))
    assert np.array_equal(out, got)
    nf = sum(eng.frames(3, n) for n in lens)
    mag = np.full((nf, 33), np.nan, np.float32)
    _capi.check(eng.ctx.lib.pk_stftd_magnitude(eng.h, 3, _capi.fptr(hx), lens.ctypes.data_as(C.POINTER(C.c_int32)), 3,
                                               _capi.fptr(mag), _capi.PK_HOST_IO))
    assert np.array_equal(mag, np.concatenate([_np(m) for m in eng.magnitude(3, xs)]))


def test_stft_matches_the_golden():
    from parakeet_amd import stft_loss as sl
    g = _gold()
    for r in lc.RESOLUTIONS:
        got = _np(sl.stft(g["x"], r.n_fft, r.hop, r.win, "hann"))
        want = g["mag_x_" + lc.res_id(r)]
        assert got.shape == want.shape
        q = max(fb.ratio(got[b], want[b], lr.Field(g["x"][b], r).b_X) for b in range(2))
        print(f"SWEEP-RATIO stft_loss engine stft golden {lc.res_id(r)} {q:.4f}")
        assert q <= 1.0


def _golden_bounds(rs):
    g = _gold()
    parts = []
    for r in rs:
        per = [lr.sums_with_bound(x, y, r) for x, y in zip(g["x"], g["y"])]
        parts.append(lr.loss_bounds(sum(p[0] for p in per), sum(p[1] for p in per), sum(p[2].X.size for p in per)))
    return np.mean([p[2] for p in parts]), np.mean([p[3] for p in parts])


def test_multi_resolution_defaults_match_the_golden():
    from parakeet_amd import stft_loss as sl
    g = _gold()
    b_sc, b_mag = _golden_bounds(lc.RECIPE)
    crit = sl.MultiResolutionSTFTLoss()
    for key, x, y in (("multi_resolution", g["x"], g["y"]),
                      ("multi_resolution_bct", g["x"].reshape(1, 2, -1), g["y"].reshape(1, 2, -1))):
        sc, mag = crit(torch.from_numpy(x), torch.from_numpy(y))
        assert sc.dim() == 0 and mag.dim() == 0 and sc.is_cuda
        rs, rm = crit.resolution_losses(x, y)
        q = max(abs(rs.mean() - g[key][0]) / b_sc, abs(rm.mean() - g[key][1]) / b_mag)
        print(f"SWEEP-RATIO stft_loss engine {key} {q:.4f} sc={float(sc):.6f} mag={float(mag):.6f}")
        assert q <= 1.0
        assert float(sc) == np.float32(rs.mean()) and float(mag) == np.float32(rm.mean())


def test_stft_loss_single_resolution_matches_the_golden():
    from parakeet_amd import stft_loss as sl
    g = _gold()
    i = lc.RESOLUTIONS.index(lc.Res(512, 50, 240))
    b_sc, b_mag = _golden_bounds([lc.RESOLUTIONS[i]])
    sc, mag = sl.STFTLoss(512, 50, 240)(g["x"], g["y"])
    assert abs(float(sc) - g["stft_loss"][i, 0]) <= b_sc + 2 * fb.U * float(sc)      # + the float32 of the 0-d tensor
    assert abs(float(mag) - g["stft_loss"][i, 1]) <= b_mag + 2 * fb.U * float(mag)


def test_identical_signals_give_zero_and_swapping_changes_sc_only():
    from parakeet_amd import stft_loss as sl
    g = _gold()
    crit = sl.MultiResolutionSTFTLoss()
    sc, mag = crit(g["y"], g["y"])
    assert float(sc) == 0.0 and float(mag) == 0.0
    a, b = crit.resolution_losses(g["x"], g["y"]), crit.resolution_losses(g["y"], g["x"])
    assert np.array_equal(a[1], b[1])                       # |ln Y - ln X| is symmetric, bit for bit
    assert (a[0] != b[0]).all() and float(crit(g["x"], g["y"])[0]) != float(crit(g["y"], g["x"])[0])


def test_sums_do_not_depend_on_the_batch():
    """An utterance's sums are bit-identical alone, first and last in a ragged batch; a second run repeats the first."""
    for r in (lc.RESOLUTIONS[2], lc.RESOLUTIONS[3], lc.RESOLUTIONS[4]):
        xs, ys = lc.batch(r)
        xs[1] = (0.5 * ys[1][::-1]).copy()                  # no silence here: every utterance has terms of its own
        eng = _eng((r,))
        whole = eng.sums(xs, ys)
        assert np.array_equal(whole, eng.sums(xs, ys))
        for b in range(3):
            alone = eng.sums([xs[b]], [ys[b]])[0]
            o = [i for i in range(3) if i != b]
            first = eng.sums([xs[b]] + [xs[i] for i in o], [ys[b]] + [ys[i] for i in o])[0]
            last = eng.sums([xs[i] for i in o] + [xs[b]], [ys[i] for i in o] + [ys[b]])[-1]
            assert np.array_equal(alone, whole[b]) and np.array_equal(alone, first) and np.array_equal(alone, last)
            assert (alone > 0).all()


def test_scaling_by_a_power_of_two_is_exact():
    """No entry at the floor: 2^+-20 on both signals is 2^+-40 on the first two sums, exactly."""
    r = lc.RESOLUTIONS[4]
    xs, ys = lc.loud_batch(r)
    for v in xs + ys:                                       # the precondition, on the fp64 reference, at the small end
        f = lr.Field(v.astype(np.float64) * 2.0 ** -20, r)
        assert ((f.X - f.b_X) ** 2 > 4.0 * lr.POWER_FLOOR).all()
    eng = _eng((r,))
    base = eng.sums(xs, ys)
    for e in (-20, 20):
        k = np.float32(2.0 ** e)
        got = eng.sums([x * k for x in xs], [y * k for y in ys])
        assert np.array_equal(got[..., :2], base[..., :2] * 2.0 ** (2 * e)), e
        assert np.isfinite(got).all() and (got[..., :2] > 0).all()


def test_per_utterance_equals_the_batch_of_one():
    from parakeet_amd import stft_loss as sl
    crit = sl.MultiResolutionSTFTLoss([64, 32, 512], [7, 6, 50], [30, 20, 240])
    xs, ys = lc.batch(lc.RESOLUTIONS[4])
    got = crit.per_utterance(xs, ys)
    assert got.shape == (3, 3, 2)
    for b in range(3):
        sc, mag = crit.resolution_losses(xs[b][None], ys[b][None])
        assert np.array_equal(got[b, :, 0], sc) and np.array_equal(got[b, :, 1], mag)
    with pytest.raises(ValueError):
        crit.per_utterance(xs, [ys[0], ys[1], ys[2][:-1]])
    with pytest.raises(ValueError):
        crit.per_utterance(xs, ys[:2])


def test_losses_on_given_magnitudes_match_numpy():
    from parakeet_amd import stft_loss as sl
    g = lc.rng_for("given magnitudes")
    x = np.abs(g.standard_normal((2, 37, 33))).astype(np.float32) * 10.0 ** g.uniform(-9, 1, (2, 37, 33)).astype(np.float32)
    y = np.abs(g.standard_normal((2, 37, 33))).astype(np.float32)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    sc = sl.SpectralConvergenceLoss()(xd, yd)
    mag = sl.LogSTFTMagnitudeLoss(1e-7)(xd, yd)
    assert sc.is_cuda and mag.is_cuda
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    n = x.size
    assert abs(float(sc) - lr.spectral_convergence(x64, y64)) <= (n + 8) * fb.U * lr.spectral_convergence(x64, y64)
    want = lr.log_stft_magnitude(x64, y64)
    # logf 2 ulp on values up to |ln 1e-7| = 16.2 on both sides, the subtraction, the mean of n terms
    assert abs(float(mag) - want) <= 2 * 4 * fb.U * 16.2 + (n + 8) * fb.U * want
    z = torch.zeros_like(yd)
    assert float(sl.SpectralConvergenceLoss()(z, z)) == 0.0


def test_refusals():
    from parakeet_amd import stft_loss as sl
    from parakeet_amd.audio import _Engine
    x = np.zeros((1, 4000), np.float32)
    with pytest.raises(NotImplementedError):
        sl.stft(x, 1000, 250, 1000)
    with pytest.raises(NotImplementedError):
        sl.MultiResolutionSTFTLoss([1000], [250], [1000])
    with pytest.raises(ValueError):
        sl.stft(x[:, :256], 512, 50, 240)                   # needs more than n_fft / 2 samples
    with pytest.raises(ValueError):
        sl.MultiResolutionSTFTLoss()(x[:, :1024], x[:, :1024])
    with pytest.raises(ValueError):
        sl.MultiResolutionSTFTLoss()(x, x[:, :-1])
    with pytest.raises(NotImplementedError):
        _Engine(1024, 250, 1024, "hann", True, False, None, 0)          # the feature path keeps its limit
    # more candidate frames than the row index holds: refused before anything is sized or touched
    eng1 = sl._DistEngine([16], [1], [16])
    many = np.full(600, 1000000, np.int32)
    rc = eng1.ctx.lib.pk_stftd_run(eng1.h, C.c_void_p(8), C.c_void_p(8), many.ctypes.data_as(C.POINTER(C.c_int32)), 600,
                                   C.c_void_p(8), 0)
    assert rc == -3 and b"too many frames" in eng1.ctx.lib.pk_last_error()
    # an uncentred transform longer than the signal has no frame: no NaN, an error
    short = sl._DistEngine([64], [16], [64], center=False)
    with pytest.raises(ValueError):
        sl.losses_from_sums(short.sums([x[0, :40]], [x[0, :40]]), short.entries([40]))
    # the cache of handles is bounded and can be emptied
    for hop in range(1, sl.MAX_CACHED_ENGINES + 3):
        sl.stft(x[:, :200], 32, hop, 32)
    assert len(sl._ENGINES) == sl.MAX_CACHED_ENGINES
    sl.clear_cache()
    assert len(sl._ENGINES) == 0
    eng = _eng((lc.RESOLUTIONS[0],))
    lens = np.array([100], np.int32)
    for args in ((None, 1), (C.c_void_p(8), 0)):
        rc = eng.ctx.lib.pk_stftd_run(eng.h, args[0], C.c_void_p(8), lens.ctypes.data_as(C.POINTER(C.c_int32)), args[1],
                                      C.c_void_p(8), 0)
        assert rc == -1 and eng.ctx.lib.pk_last_error()
