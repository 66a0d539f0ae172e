"""The pseudo-QMF bank on the engine (csrc/pqmf.hip) against the fp64 restatement of tests/pqmf_ref.py: analysis and
synthesis within the bound derived with fp32_bounds.dot_bound for the products an output really sums, over banks (K, taps) =
(4, 62), (2, 6), (3, 14) and lengths from one band sample -- fewer than taps / (2 K), so that both ends of the filter hang
over the utterance -- to ends at -1, 0, +1 and +2 of the kernels' 256-output tiles; the same bits in any batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import fp32_bounds as fb  # noqa: E402
import pqmf_ref as pr  # noqa: E402

from parakeet_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

# band samples per utterance.  Analysis tiles 256 band samples; synthesis tiles 256 = K M output samples:
#   K = 4: M = 63, 64, 65 end 4 before, at and 4 past a synthesis tile (a length is a multiple of K); 255 ... 258 the analysis tile
#   K = 2: M = 127, 128, 129 (-2, 0, +2);   K = 3: M = 85 (255: -1), 86 (258: +2), 171 (513: +1), 256 (768: 0), 341 (1023: -1)
BANKS = {(4, 62): (0.142, 9.0, (1, 3, 7, 63, 64, 65, 255, 256, 257, 258)),
         (2, 6): (0.25, 4.0, (1, 2, 127, 128, 129, 255, 256, 257)),
         (3, 14): (0.2, 6.0, (1, 2, 85, 86, 171, 256, 257, 341))}


def host(t):
    return t.as_subclass(torch.Tensor).cpu().numpy()


def bank(K, taps):
    from parakeet_amd.melgan import PQMF
    cutoff, beta, Ms = BANKS[(K, taps)]
    return PQMF(subbands=K, taps=taps, cutoff_ratio=cutoff, beta=beta), cutoff, beta, Ms


@pytest.mark.parametrize("K,taps", list(BANKS))
def test_filters_are_the_restatement(K, taps):
    q, cutoff, beta, _ = bank(K, taps)
    ana, syn = q.filters()
    want_a, want_s = pr.filters(K, taps, cutoff, beta)
    for got, want, name in ((ana, want_a, "analysis"), (syn, want_s, "synthesis")):
        r = fb.ratio(got, want, pr.filter_tolerance(want))
        print(f"SWEEP-RATIO pqmf K={K} taps={taps} {name} filter: {r:.3g}")
        assert r <= 1.0


@pytest.mark.parametrize("K,taps", list(BANKS))
def test_analysis_and_synthesis_within_derived_bounds(K, taps):
    q, _, _, Ms = bank(K, taps)
    ana, syn = (f.astype(np.float64) for f in q.filters())
    rng = np.random.default_rng(K * 100 + taps)
    lens = [K * M + (b % K) for b, M in enumerate(Ms)]          # floor(L / K) = M with every remainder
    wavs = [rng.standard_normal(L).astype(np.float32) for L in lens]
    got = host(q.analysis_packed(np.concatenate(wavs), lens))
    bands, o, worst_a = [], 0, 0.0
    for x, M in zip(wavs, Ms):
        blk = got[o:o + K * M].reshape(K, M)
        o += K * M
        want, bound = pr.analysis(x, ana)
        worst_a = max(worst_a, fb.ratio(blk, want, bound))
        bands.append(blk)
    assert o == got.size
    # synthesis of the engine's own bands
    wav = host(q.synthesis_packed(np.concatenate([b.reshape(-1) for b in bands]), list(Ms)))
    o, worst_s = 0, 0.0
    for blk, M in zip(bands, Ms):
        want, bound = pr.synthesis(blk, syn)
        worst_s = max(worst_s, fb.ratio(wav[o:o + K * M], want, bound))
        o += K * M
    assert o == wav.size
    print(f"SWEEP-RATIO pqmf K={K} taps={taps}: analysis={worst_a:.3g} ({taps + 1} products) synthesis={worst_s:.3g} "
          f"({pr.nprod_synthesis(K, taps)} products)")
    assert worst_a <= 1.0 and worst_s <= 1.0
    # the same bits alone, reversed, and through the (N, 1, T) / (N, K, M) entry points
    rev_a = host(q.analysis_packed(np.concatenate(wavs[::-1]), lens[::-1]))
    rev_s = host(q.synthesis_packed(np.concatenate([b.reshape(-1) for b in bands[::-1]]), list(Ms[::-1])))
    oa = os_ = 0
    for x, blk, M in list(zip(wavs, bands, Ms))[::-1]:
        np.testing.assert_array_equal(rev_a[oa:oa + K * M].reshape(K, M), blk)
        np.testing.assert_array_equal(host(q.analysis(x)), blk)
        alone = host(q.synthesis(blk))
        np.testing.assert_array_equal(rev_s[os_:os_ + K * M], alone)
        oa += K * M
        os_ += K * M
    o = 0
    for blk, M in zip(bands, Ms):
        np.testing.assert_array_equal(wav[o:o + K * M], host(q.synthesis(blk)))
        o += K * M
    two = host(q.analysis(np.stack([wavs[-1], wavs[-1]])[:, None, :]))
    assert two.shape == (2, K, Ms[-1])
    np.testing.assert_array_equal(two[1], bands[-1])
    np.testing.assert_array_equal(host(q.synthesis(two))[0, 0], host(q.synthesis(bands[-1])))


def test_c_abi_host_pointers_and_refusals():
    q, _, _, _ = bank(4, 62)
    ctx = q._engine()
    lib = ctx.lib
    x = np.random.default_rng(1).standard_normal(1030).astype(np.float32)
    want = host(q.analysis(x))
    lens = np.array([1030], np.int32)
    out = np.empty(4 * 257, np.float32)
    i32p = C.POINTER(C.c_int32)
    _capi.check(lib.pk_pqmf_analysis(q._h, _capi.fptr(x), lens.ctypes.data_as(i32p), 1, _capi.fptr(out), _capi.PK_HOST_IO))
    np.testing.assert_array_equal(out.reshape(4, 257), want)
    wav = np.empty(1028, np.float32)
    bl = np.array([257], np.int32)
    _capi.check(lib.pk_pqmf_synthesis(q._h, _capi.fptr(out), bl.ctypes.data_as(i32p), 1, _capi.fptr(wav), _capi.PK_HOST_IO))
    np.testing.assert_array_equal(wav, host(q.synthesis(want)))
    # the bank's own reconstruction error, not a check of the arithmetic: printed
    print(f"SWEEP-RATIO pqmf K=4 taps=62 reconstruction error / peak away from the ends: "
          f"{np.abs(wav - x[:1028])[128:-128].max() / np.abs(x).max():.3g}")
    short = np.array([3], np.int32)
    assert lib.pk_pqmf_analysis(q._h, _capi.fptr(x), short.ctypes.data_as(i32p), 1, _capi.fptr(out), 1) == -1
    zero = np.array([0], np.int32)
    assert lib.pk_pqmf_synthesis(q._h, _capi.fptr(out), zero.ctypes.data_as(i32p), 1, _capi.fptr(wav), 1) == -1
    assert lib.pk_pqmf_analysis(q._h, _capi.fptr(x), lens.ctypes.data_as(i32p), 0, _capi.fptr(out), 1) == -1
    h = C.c_void_p()
    for bad in (_capi.PqmfCfg(1, 62, 0.142, 9.0), _capi.PqmfCfg(17, 62, 0.142, 9.0), _capi.PqmfCfg(4, 63, 0.142, 9.0),
                _capi.PqmfCfg(4, 256, 0.142, 9.0), _capi.PqmfCfg(4, 62, 0.5, 9.0), _capi.PqmfCfg(4, 62, 0.142, -1.0)):
        assert lib.pk_pqmf_create(ctx.handle, C.byref(bad), C.byref(h)) == -3 and not h
    buf = np.empty(5, np.float32)
    assert lib.pk_pqmf_filters(q._h, _capi.fptr(buf), _capi.fptr(buf), buf.size) == -2
