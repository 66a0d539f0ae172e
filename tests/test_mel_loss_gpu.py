"""Masked L1 and SSIM of mel pairs on the engine (csrc/mel_loss.hip, parakeet_amd/ssim.py, parakeet_amd/losses.py) against
the float64 restatement of tests/mel_loss_ref.py.

Bounds.  Map, per pixel: |engine - float64| <= 4 x the reference's own float32 deviation for that case
(``ssim_ref_dev_<case>`` of tests/golden/speedyspeech_forward.npz; the factor 4 because the separable pass rounds in another
order than the 121-tap sum).  Map sum: the same bound on the mean.  L1 sum: relative 1e-6, a float32 |a - b| summed in
float64.  ``SWEEP-RATIO`` lines give error / bound."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import mel_loss_cases as mc
import mel_loss_ref as mr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(GOLD, "speedyspeech_forward.npz")))


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("c", mc.CASES, ids=mc.case_id)
def test_map_and_sums_match_the_restatement(c):
    from parakeet_amd.losses import mel_loss_sums
    p, t = mc.pair(c)
    rows = c.L + c.pad
    l1, m64 = mr.pair_sums(p, t, rows, c.ws)
    bound = 4.0 * float(_gold()["ssim_ref_dev_" + mc.case_id(c)])
    sums, m = mel_loss_sums(p, t, [c.L], padded=[rows], window_size=c.ws, return_map=True)
    m = _np(m)
    assert m.shape == (rows, c.W) and sums.shape == (1, 2) and sums.dtype == np.float64
    q_map = np.abs(m.astype(np.float64) - m64).max() / bound
    q_sum = abs(sums[0, 1] / m64.size - m64.mean()) / bound
    q_l1 = abs(sums[0, 0] - l1) / (1e-6 * l1)
    print(f"SWEEP-RATIO mel_loss engine {mc.case_id(c)} map {q_map:.4f} map-sum {q_sum:.4f} l1 {q_l1:.4f}")
    assert q_map <= 1.0 and q_sum <= 1.0 and q_l1 <= 1.0
    if c.pad > c.ws // 2:                                   # rows no window reaches from: exactly 1
        assert (m[c.L + c.ws // 2:] == 1.0).all()
    without = mel_loss_sums(p, t, [c.L], padded=[rows], window_size=c.ws)
    assert np.array_equal(without, sums)                     # ssim_map_out = NULL changes nothing


def test_ragged_batch_equals_every_pair_alone_bit_for_bit():
    from parakeet_amd.losses import mel_loss_sums
    cs = [c for c in mc.CASES if c.W == 80 and c.ws == 11 and c.kind == "raw"][:5]
    assert len(cs) == 5
    pairs = [mc.pair(c) for c in cs]
    lens, pads = [c.L for c in cs], [c.L + c.pad for c in cs]
    whole, wmap = mel_loss_sums(np.concatenate([p for p, _ in pairs]), np.concatenate([t for _, t in pairs]), lens, padded=pads,
                                return_map=True)
    assert np.array_equal(whole, mel_loss_sums(np.concatenate([p for p, _ in pairs]), np.concatenate([t for _, t in pairs]),
                                               lens, padded=pads))
    o = 0
    for b, (p, t) in enumerate(pairs):
        alone, amap = mel_loss_sums(p, t, [lens[b]], padded=[pads[b]], return_map=True)
        assert np.array_equal(alone[0], whole[b]) and (alone[0] > 0).all()
        assert np.array_equal(_np(amap), _np(wmap)[o:o + pads[b]])
        o += pads[b]
    rev = mel_loss_sums(np.concatenate([p for p, _ in pairs[::-1]]), np.concatenate([t for _, t in pairs[::-1]]), lens[::-1],
                        padded=pads[::-1])
    assert np.array_equal(rev[::-1], whole)


def test_wide_images_are_tiled_by_columns():
    """W = 200 and 1024: more than one column tile, the halo columns come from the neighbouring tile."""
    from parakeet_amd.losses import mel_loss_sums
    g = mc.rng_for("wide")
    for W, L in ((200, 19), (1024, 5)):
        t = g.standard_normal((L, W)).astype(np.float32)
        p = (t + 0.1 * g.standard_normal((L, W))).astype(np.float32)
        l1, m64 = mr.pair_sums(p, t, L + 2, 11)
        dev = np.abs(mr.ssim_map(mc.padded(p, L + 2), mc.padded(t, L + 2), 11, torch.float32).astype(np.float64) - m64).max()
        sums, m = mel_loss_sums(p, t, [L], padded=[L + 2], return_map=True)
        assert np.abs(_np(m).astype(np.float64) - m64).max() <= 4 * dev
        assert abs(sums[0, 0] - l1) <= 1e-6 * l1 and abs(sums[0, 1] / m64.size - m64.mean()) <= 4 * dev


def test_python_surface_ssim_and_masked_l1():
    from parakeet_amd import losses, ssim
    g = mc.rng_for("surface")
    a = g.standard_normal((2, 2, 9, 12)).astype(np.float32)
    b = (a + 0.1 * g.standard_normal(a.shape)).astype(np.float32)
    want = mr.ssim(a, b, 3, size_average=False)
    got = ssim.ssim(torch.from_numpy(a), torch.from_numpy(b), 3, size_average=False)
    assert got.shape == (2,) and np.abs(_np(got) - want).max() < 1e-5
    assert abs(float(ssim.ssim(a, b, 3)) - want.mean()) < 1e-5
    assert abs(float(ssim.SSIM(3)(a, b)) - want.mean()) < 1e-5
    assert float(ssim.ssim(a, a)) == 1.0                     # an image with itself
    per = ssim.ssim_per_pair([a[0, 0], a[1, 1][:5]], [b[0, 0], b[1, 1][:5]], 3)
    assert abs(per[0] - mr.ssim(a[:1, :1], b[:1, :1], 3)) < 1e-5
    assert abs(per[1] - mr.ssim(a[1:, 1:, :5], b[1:, 1:, :5], 3)) < 1e-5
    x, y = a.reshape(4, 9, 12), b.reshape(4, 9, 12)
    mask = mr.sequence_mask([9, 4, 1, 7], 9)[:, :, None].astype(np.float32)
    want = mr.masked_l1_loss(x, y, mask)
    got = losses.masked_l1_loss(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(mask))
    assert got.dim() == 0 and abs(float(got) - want) <= 2e-6 * want
    assert abs(float(losses.weighted_mean(torch.from_numpy(np.abs(x - y)), torch.from_numpy(mask))) - want) <= 1e-5 * want
    with pytest.raises(NotImplementedError, match="frame mask"):
        losses.masked_l1_loss(x, y, np.ones((4, 9, 12), np.float32))
    holes = mask.copy()
    holes[0, 3] = 0
    with pytest.raises(NotImplementedError, match="prefix form"):
        losses.masked_l1_loss(x, y, holes)


def test_refusals_and_host_io():
    from parakeet_amd import _capi
    from parakeet_amd.losses import mel_loss_sums
    from parakeet_amd.runtime import Context
    c = mc.CASES[2]
    p, t = mc.pair(c)
    for ws in (0, 2, 10, -1):
        with pytest.raises(ValueError, match="odd"):
            mel_loss_sums(p, t, [c.L], window_size=ws)
    with pytest.raises(NotImplementedError):
        mel_loss_sums(p, t, [c.L], window_size=35)
    with pytest.raises(NotImplementedError):
        mel_loss_sums(np.zeros((1, 1025), np.float32), np.zeros((1, 1025), np.float32), [1])
    with pytest.raises(ValueError, match="padded_lens"):
        mel_loss_sums(p, t, [c.L], padded=[c.L - 1])
    ctx = Context.get()
    lens, pads = np.array([c.L], np.int32), np.array([c.L + c.pad], np.int32)
    i32p = C.POINTER(C.c_int32)
    out = np.full((1, 2), np.nan)
    m = np.full((c.L + c.pad, c.W), np.nan, np.float32)
    _capi.check(ctx.lib.pk_mel_loss_run(ctx.handle, _capi.fptr(p), _capi.fptr(t), lens.ctypes.data_as(i32p),
                                        pads.ctypes.data_as(i32p), 1, c.W, c.ws, out.ctypes.data_as(C.c_void_p), _capi.fptr(m),
                                        _capi.PK_HOST_IO))
    sums, dm = mel_loss_sums(p, t, lens, padded=pads, window_size=c.ws, return_map=True)
    assert np.array_equal(out, sums) and np.array_equal(m, _np(dm))
    rc = ctx.lib.pk_mel_loss_run(ctx.handle, None, _capi.fptr(t), lens.ctypes.data_as(i32p), None, 1, c.W, c.ws,
                                 out.ctypes.data_as(C.c_void_p), None, _capi.PK_HOST_IO)
    assert rc == -1 and ctx.lib.pk_last_error()
