"""The pseudo-QMF bank without a device: the restatement (tests/pqmf_ref.py) against numpy.correlate / zero insertion and
numpy.kaiser, the bank's own reconstruction error, and the proof that the derived bound tells a wrong kernel from a right one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fp32_bounds as fb  # noqa: E402
import pqmf_ref as pr  # noqa: E402

BANKS = [(4, 62, 0.142, 9.0), (2, 6, 0.25, 4.0), (3, 14, 0.2, 6.0), (16, 254, 0.035, 12.0)]


@pytest.mark.parametrize("M,beta", [(63, 9.0), (7, 0.0), (15, 6.0), (255, 14.0), (5, 100.0)])
def test_kaiser_equals_numpy(M, beta):
    np.testing.assert_allclose(pr.kaiser(M, beta), np.kaiser(M, beta), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("K,taps,cutoff,beta", BANKS)
def test_restatement_equals_correlate(K, taps, cutoff, beta):
    ana, syn = pr.filters(K, taps, cutoff, beta)
    assert ana.shape == syn.shape == (K, taps + 1)
    np.testing.assert_array_equal(ana, ana.astype(np.float32).astype(np.float64))
    # the centre tap of the prototype is cutoff: analysis_k[taps / 2] = 2 cutoff cos(+- pi / 4)
    np.testing.assert_allclose(np.abs(ana[:, taps // 2]), 2 * np.float32(cutoff) * np.cos(np.pi / 4), rtol=1e-6)
    rng = np.random.default_rng(K * 1000 + taps)
    for L in (K, K + 1, 3 * K - 1, taps // 2, taps + 3, 5 * taps + K + 1):
        if L < K:
            continue
        x = rng.standard_normal(L)
        bands, bound = pr.analysis(x, ana)
        assert bands.shape == (K, L // K) == bound.shape
        np.testing.assert_allclose(bands, pr.analysis_correlate(x, ana), rtol=0, atol=1e-13)
        wav, bound = pr.synthesis(bands, syn)
        assert wav.shape == (K * (L // K),) == bound.shape
        np.testing.assert_allclose(wav, pr.synthesis_correlate(bands, syn), rtol=0, atol=1e-12)


def test_reconstruction_error_of_the_default_bank():
    """Analysis followed by synthesis reproduces a signal to 8e-4 of its peak away from the ends: the bank's own error."""
    ana, syn = pr.filters(4, 62, 0.142, 9.0)
    t = np.arange(4096)
    x = 0.5 * np.sin(2 * np.pi * 0.013 * t) + 0.3 * np.sin(2 * np.pi * 0.21 * t + 1.0) + 0.1 * np.random.default_rng(0).standard_normal(4096)
    y = pr.synthesis(pr.analysis(x, ana, False)[0], syn, False)[0]
    err = np.abs(y - x)[128:-128].max() / np.abs(x).max()
    print(f"PQMF reconstruction error / peak away from the ends: {err:.3g}")
    assert err < 8e-4


@pytest.mark.parametrize("K,taps,cutoff,beta", BANKS[:3])
def test_bound_is_not_vacuous(K, taps, cutoff, beta):
    """The restatement rounded to float32 stays far inside the bound; a dropped tap, a filter shifted by one sample, the
    analysis filter used for synthesis, and a missing factor K leave it."""
    ana, syn = pr.filters(K, taps, cutoff, beta)
    x = np.random.default_rng(3).standard_normal(11 * taps + 5).astype(np.float32)
    bands, b_a = pr.analysis(x, ana)
    assert fb.ratio(bands.astype(np.float32), bands, b_a) < 0.5
    drop = ana.copy()
    drop[np.arange(K), np.abs(ana[:, :taps // 2]).argmax(1)] = 0.0   # each band's largest tap left of the centre
    assert fb.ratio(pr.analysis(x, drop, False)[0], bands, b_a) > 1.0
    assert fb.ratio(pr.analysis(x, np.roll(ana, 1, axis=1), False)[0], bands, b_a) > 1.0
    b32 = bands.astype(np.float32)
    wav, b_s = pr.synthesis(b32, syn)
    assert fb.ratio(wav.astype(np.float32), wav, b_s) < 0.5
    assert fb.ratio(pr.synthesis(b32, ana, False)[0], wav, b_s) > 1.0
    assert fb.ratio(wav / K, wav, b_s) > 1.0
    assert fb.ratio(pr.synthesis(b32, np.roll(syn, 1, axis=1), False)[0], wav, b_s) > 1.0
    print(f"PQMF K={K} taps={taps}: analysis bound / peak {b_a.max() / np.abs(bands).max():.3g}, synthesis {b_s.max() / np.abs(wav).max():.3g}")
