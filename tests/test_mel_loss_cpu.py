"""The float64 restatement of ssim.py / losses.py (tests/mel_loss_ref.py) against the reference's own float32 maps
(tests/golden/speedyspeech_forward.npz), the properties the engine tests rely on, and the new modules' surface."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import mel_loss_cases as mc
import mel_loss_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(GOLD, "speedyspeech_forward.npz")))


def test_cases_cover_what_the_issue_lists():
    T = mc.ROW_TILE
    assert {c.W for c in mc.CASES} == {1, 5, 80}
    assert {c.L for c in mc.CASES} == {1, 7, T - 1, T, T + 1, 2 * T + 3}
    assert {c.ws for c in mc.CASES} == {1, 3, 11}
    assert {c.kind for c in mc.CASES} == {"z", "raw"}
    assert {0, 1, 13} <= {c.pad for c in mc.CASES} and any(c.pad == c.ws // 2 and c.pad > 1 for c in mc.CASES)
    assert max((c.L + c.pad) * c.W for c in mc.CASES) <= 50 * 80
    from parakeet_amd import _capi
    header = open(os.path.join(ROOT, "parakeet_amd", "csrc", "pk_mel_loss.h")).read()
    assert int(re.search(r"#define PK_MEL_LOSS_ROWS (\d+)", header).group(1)) == _capi.PK_MEL_LOSS_ROWS == T


@pytest.mark.parametrize("c", mc.CASES, ids=mc.case_id)
def test_restatement_in_float32_is_the_reference_and_float32_stays_close_to_float64(c):
    g = _gold()
    p, t = mc.pair(c)
    a, b = mc.padded(p, c.L + c.pad), mc.padded(t, c.L + c.pad)
    ref32 = g["ssim_map_" + mc.case_id(c)]
    assert ref32.shape == (c.L + c.pad, c.W) and ref32.dtype == np.float32
    m64 = mr.ssim_map(a, b, c.ws)
    dev = float(g["ssim_ref_dev_" + mc.case_id(c)])
    assert float(np.abs(ref32.astype(np.float64) - m64).max()) == dev
    assert 0.0 < dev < 2e-5                                                   # the reference's own float32, per pixel
    # the restatement run in float32 is the reference's arithmetic (same operators, same order)
    assert np.abs(mr.ssim_map(a, b, c.ws, torch.float32) - ref32).max() <= 4 * dev
    l1, m = mr.pair_sums(p, t, c.L + c.pad, c.ws)
    assert np.array_equal(m, m64) and l1 == np.abs(p.astype(np.float64) - t.astype(np.float64)).sum()


def test_an_image_with_itself_scores_exactly_one():
    for c in mc.CASES[:4] + mc.CASES[-4:]:
        _, t = mc.pair(c)
        assert (mr.ssim_map(t, t, c.ws) == 1.0).all()
        assert mr.ssim(t[None, None], t[None, None], c.ws) == 1.0


def test_rows_out_of_the_windows_reach_are_exactly_one():
    for c in mc.CASES:
        if c.pad > c.ws // 2:
            p, t = mc.pair(c)
            _, m = mr.pair_sums(p, t, c.L + c.pad, c.ws)
            far = c.L - 1 + c.ws // 2 + 1                                     # first row whose window holds no valid row
            assert far < c.L + c.pad and (m[far:] == 1.0).all()
            assert (m[far - 1] != 1.0).any() or c.ws == 1


def test_channels_are_independent_images():
    g = mc.rng_for("two channels")
    a = g.standard_normal((2, 2, 9, 12))
    b = a + 0.1 * g.standard_normal(a.shape)
    both = mr.ssim(a, b, 3, size_average=False)
    for i in range(2):
        sep = [mr.ssim(a[i:i + 1, ch:ch + 1], b[i:i + 1, ch:ch + 1], 3) for ch in range(2)]
        assert abs(both[i] - np.mean(sep)) < 1e-15
    assert abs(mr.ssim(a, b, 3) - both.mean()) < 1e-15


def test_weighted_mean_broadcasting_and_huber():
    g = mc.rng_for("weighted mean")
    x = g.standard_normal((3, 7, 5))
    mask = mr.sequence_mask([7, 3, 1], 7)[:, :, None]
    assert abs(mr.weighted_mean(x, mask) - (x * mask).sum() / (11 * 5)) < 1e-15
    assert abs(mr.masked_l1_loss(x, 0 * x, mask) - (np.abs(x) * mask).sum() / 55) < 1e-15
    assert np.array_equal(mr.huber([0.0, 0.0, 0.0, 0.0], [0.5, -1.0, 3.0, -1.5]), [0.125, 0.5, 2.5, 1.0])


def test_new_modules_import_and_expose_the_references_names():
    import parakeet_amd.losses as losses
    import parakeet_amd.ssim as ssim
    for name in ("gaussian", "create_window", "ssim", "SSIM", "ssim_per_pair"):
        assert hasattr(ssim, name), name
    for name in ("weighted_mean", "masked_l1_loss"):
        assert hasattr(losses, name), name
    w = ssim.gaussian(11, 1.5)
    assert w.dtype == torch.float32 and torch.equal(w, mr.gaussian(11))
    win = ssim.create_window(11, 2)
    assert tuple(win.shape) == (2, 1, 11, 11) and torch.equal(win[1, 0].double(), mr.window2d(11))
