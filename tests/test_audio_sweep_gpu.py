"""Sweep of the STFT / magnitude / power / mel / log-mel path (mel.hip: reflect padding, the STFT and filterbank products
on k_gemm with their tail tiles, the row map of a ragged batch) against an fp64 restatement of parakeet/modules/audio.py
:74-229 and parakeet/data/get_feats.py:20-88, under the derived bounds of tests/fp32_bounds.py.

One ragged batch per configuration (tests/sweep_cases.py: the shortest legal utterance, silence, a full-scale +-1 signal,
with center=False one shorter than n_fft, and a long one that crosses the 128-row tile; the frames of two batches add up to
exactly 128 and 129).  ``SWEEP-RATIO`` lines give error / bound per quantity.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fp32_bounds as fb
import sweep_cases as sc

pytestmark = pytest.mark.gpu

UP, DOWN = np.float32(2.0 ** 20), np.float32(2.0 ** -20)


def _np(t):
    return t.detach().cpu().numpy()


def _engine(c, basis=None, power=False, log_base=0):
    from parakeet_amd.audio import _Engine
    return _Engine(c.n_fft, c.hop, c.win, "hann", c.center, power, basis, log_base)


def _run(eng, wavs, what):
    return [_np(o) for o in eng.run(wavs, what)]


def _run_host(eng, wavs, what, cols):
    """pk_mel_run with PK_HOST_IO: host samples in, host result out."""
    from parakeet_amd import _capi
    lens = np.array([len(w) for w in wavs], dtype=np.int32)
    x = np.ascontiguousarray(np.concatenate(wavs), dtype=np.float32)
    out = np.full((sum(eng.frames(n) for n in lens), cols), np.nan, np.float32)
    _capi.check(eng.ctx.lib.pk_mel_run(eng.h, _capi.fptr(x), lens.ctypes.data_as(C.POINTER(C.c_int32)), len(wavs),
                                       _capi.fptr(out), what, _capi.PK_HOST_IO))
    return out


@pytest.mark.parametrize("c", sc.MEL_CFGS, ids=sc.mel_id)
def test_stft_mel_sweep(c):
    from parakeet_amd.audio import mel_filterbank
    basis = mel_filterbank(c.sr, c.n_fft, c.n_mels, sc.MEL_FMIN, sc.MEL_FMAX)
    wavs = sc.mel_batch(c)
    refs = [sc.mel_reference(c, w, basis) for w in wavs]
    refs_pow = [sc.mel_reference(c, w, basis, power=True) for w in wavs]
    e_mag, e_pow = _engine(c), _engine(c, power=True)
    e_mel, e_l10, e_ln = _engine(c, basis), _engine(c, basis, log_base=10), _engine(c, basis, log_base=2)
    nb = 1 + c.n_fft // 2

    frames = [e_mag.frames(len(w)) for w in wavs]
    assert frames == [r["frames"] for r in refs] == [sc.num_frames(c, len(w)) for w in wavs]
    assert c.total_frames is None or sum(frames) == c.total_frames
    assert c.center or 0 in frames

    got = {"reim": _run(e_mag, wavs, 0), "mag": _run(e_mag, wavs, 1), "pow": _run(e_pow, wavs, 1),
           "mel": _run(e_mel, wavs, 2), "log10": _run(e_l10, wavs, 2), "ln": _run(e_ln, wavs, 2)}
    worst = {k: 0.0 for k in got}
    unusable = 0
    for u, (r, rp) in enumerate(zip(refs, refs_pow)):
        for k in got:
            assert got[k][u].shape[0] == frames[u]
        if frames[u] == 0:
            continue
        worst["reim"] = max(worst["reim"], fb.ratio(got["reim"][u], r["reim"], r["b_reim"]))
        worst["mag"] = max(worst["mag"], fb.ratio(got["mag"][u], r["spec"], r["b_spec"]))
        worst["pow"] = max(worst["pow"], fb.ratio(got["pow"][u], rp["spec"], rp["b_spec"]))
        worst["mel"] = max(worst["mel"], fb.ratio(got["mel"][u], r["mel"], r["b_mel"]))
        worst["log10"] = max(worst["log10"], fb.ratio(got["log10"][u], r["log10"], r["b_log10"], r["usable"]))
        worst["ln"] = max(worst["ln"], fb.ratio(got["ln"][u], r["ln"], r["b_ln"], r["usable"]))
        unusable += int((~r["usable"]).sum())
    for k, v in worst.items():
        print(f"SWEEP-RATIO stft_mel {sc.mel_id(c)} {k} {v:.4g}")
    total = sum(frames) * c.n_mels
    print(f"SWEEP-INFO stft_mel {sc.mel_id(c)} entries_within_the_mel_bound_of_the_floor {unusable} of {total}")
    assert max(worst.values()) <= 1.0
    assert unusable < 0.01 * total

    # silence (utterance 1): exact zeros up to the mel stage, then the floor: one value everywhere, log10(1e-10)
    for k in ("reim", "mag", "pow", "mel"):
        assert not got[k][1].any()
    z = got["log10"][1]
    print(f"SWEEP-INFO stft_mel {sc.mel_id(c)} log10_of_silence {z[0, 0]!r}")
    assert np.array_equal(z, np.full_like(z, z[0, 0])) and abs(float(z[0, 0]) + 10.0) <= 4.0 * fb.U * 10.0
    assert np.array_equal(got["ln"][1], np.full_like(z, got["ln"][1][0, 0]))

    # every utterance of the batch equals, bit for bit, its result when run alone
    for u, w in enumerate(wavs):
        if frames[u] == 0:
            continue
        for k, (eng, what) in {"reim": (e_mag, 0), "mag": (e_mag, 1), "log10": (e_l10, 2)}.items():
            assert np.array_equal(_run(eng, [w], what)[0], got[k][u]), (k, u)

    # PK_HOST_IO output equals device output, bit for bit, for what = 0 / 1 / 2 on the same ragged batch
    for k, eng, what, cols in (("reim", e_mag, 0, 2 * nb), ("mag", e_mag, 1, nb), ("pow", e_pow, 1, nb),
                               ("log10", e_l10, 2, c.n_mels)):
        assert np.array_equal(_run_host(eng, wavs, what, cols), np.concatenate(got[k])), k

    # the fp32 path scales exactly with a power of two on the samples (the log stage does not, by definition)
    for s in (UP, DOWN):
        scaled = [w * s for w in wavs]
        for k, eng, what in (("reim", e_mag, 0), ("mag", e_mag, 1), ("mel", e_mel, 2)):
            for a, b in zip(_run(eng, scaled, what), got[k]):
                assert np.array_equal(a, b * s), (k, float(s))


def test_stft_status_codes():
    from parakeet_amd.audio import _Engine
    with pytest.raises(NotImplementedError):          # PK_EUNSUPPORTED: hop_length not a multiple of 4
        _Engine(1024, 250, 1024, "hann", True, False, None, 0)
    with pytest.raises(NotImplementedError):          # PK_EUNSUPPORTED: n_fft not a multiple of 16
        _Engine(1000, 200, 1000, "hann", True, False, None, 0)
    eng = _Engine(1024, 256, 1024, "hann", True, False, None, 0)
    with pytest.raises(ValueError):                   # PK_EINVAL: n_fft / 2 samples cannot be reflect-padded by n_fft / 2
        eng.run([np.zeros(512, np.float32)], 0)
    assert eng.run([np.ones(513, np.float32)], 0)[0].shape == (3, 2 * 513)
