"""The derived bounds of tests/fp32_bounds.py are tight enough to see a wrong kernel, for every case of the sweeps.

For each GEMM-type stage of each sweep case (the im2col product of a convolution, q.k and weights.v of attention, the
STFT and the mel filterbank products) the comparator must ACCEPT a float32 numpy evaluation of the same product and REJECT
three wrong results: one dropped product, one skipped K slab of a 128-column tile, one unstored tail row.  A case that
could not meet this would have inputs too benign for its bound (|A| . |W| huge next to the result); the cure is other
inputs, never another bound.  The derived quantities (softmax weights, magnitude, log-mel) must accept their float32
evaluation too.  The covering properties the sweeps promise are asserted here as well.
"""
import itertools
import math

import numpy as np
import pytest

import fp32_bounds as fb
import sweep_cases as sc


def _check_stage(name, A, W, y, absprod, K, bias=None):
    bound = fb.dot_bound(absprod, K, bias)
    y32 = A.astype(np.float32) @ W.astype(np.float32)
    if bias is not None:
        y32 = y32 + bias.astype(np.float32)
    r = fb.ratio(y32, y, bound)
    assert r <= 1.0, f"{name}: the float32 evaluation is outside the bound (ratio {r:.3g})"
    for mname, wrong in fb.mutants(A, W, y).items():
        assert fb.ratio(wrong, y, bound) > 1.0, f"{name}: the bound accepts the '{mname}' mutant"
    return r


@pytest.mark.parametrize("c", sc.ATT_CASES + [sc.ATT_LDS_EDGE], ids=sc.att_id)
def test_attention_bounds(c):
    q, k, v, mask = sc.attention_inputs(c)
    ref = sc.attention_reference(q, k, v, mask)
    for st in ref["stages"]:
        _check_stage(*st)
    s = np.einsum("bqc,bkc->bqk", q, k) * np.float32(1.0 / np.sqrt(np.float32(c.d)))
    if mask is not None:
        s = s + (np.float32(1.0) - np.broadcast_to(mask, s.shape)) * np.float32(-1e9)
    e = np.exp(s - s.max(-1, keepdims=True))
    w = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    out = np.einsum("bqk,bkc->bqc", w, v)
    assert w.dtype == out.dtype == np.float32
    assert fb.ratio(w, ref["w"], ref["b_w"]) <= 1.0
    assert fb.ratio(out, ref["out"], ref["b_out"]) <= 1.0
    if ref["dead"].any():                                    # the fully masked row: exactly uniform in float32
        assert np.array_equal(w[ref["dead"]], np.full_like(w[ref["dead"]], np.float32(1.0) / np.float32(c.Tk)))
    # a softmax that forgets one key of a lane's second pass (Tk > 64) must be seen
    wrong = ref["w"].copy()
    wrong[..., -1] = 0.0
    if not np.array_equal(wrong, ref["w"]):
        assert fb.ratio(wrong, ref["w"], ref["b_w"]) > 1.0


@pytest.mark.parametrize("c", sc.CONV_CASES, ids=sc.conv_id)
def test_conv_bounds(c):
    x, st = sc.conv_inputs(c)
    want, bound, A, W, sh = sc.conv_reference(x, st, c.k, c.pad)
    assert want.shape == (c.B, c.T + 2 * c.pad - c.k + 1, c.Cout)
    _check_stage("conv", A, W, want.reshape(A.shape[0], -1), np.abs(A) @ np.abs(W), c.Cin * c.k, sh)


@pytest.mark.parametrize("c", sc.MM_CASES, ids=sc.mm_id)
def test_matmul_bounds(c):
    x, w, b = sc.matmul_inputs(c)
    want, _ = sc.matmul_reference(x, w, b)
    A, W = x.astype(np.float64), w.astype(np.float64)
    _check_stage("matmul", A, W, want, np.abs(A) @ np.abs(W), c.K, None if b is None else b.astype(np.float64))


@pytest.mark.parametrize("c", sc.CELL_CASES, ids=sc.cell_id)
def test_cell_bounds(c):
    x, st = sc.cell_inputs(c)
    want, _, A, W, b = sc.cell_reference(x, st, c.k, c.dil)
    y = want.transpose(0, 2, 1).reshape(A.shape[0], c.Cout)
    _check_stage("cell", A, W, y, np.abs(A) @ np.abs(W), c.Cin * c.k, b)


@pytest.mark.parametrize("c", sc.MEL_CFGS, ids=sc.mel_id)
def test_stft_mel_bounds(c):
    from parakeet_amd.audio import mel_filterbank
    basis = mel_filterbank(c.sr, c.n_fft, c.n_mels, sc.MEL_FMIN, sc.MEL_FMAX)
    wavs = sc.mel_batch(c)
    refs = [sc.mel_reference(c, w, basis) for w in wavs]
    assert [r["frames"] for r in refs] == [sc.num_frames(c, len(w)) for w in wavs]
    if c.total_frames:
        assert sum(r["frames"] for r in refs) == c.total_frames
    if not c.center:
        assert 0 in [r["frames"] for r in refs]
    # the GEMM rows of the batch, frames of all utterances in order: the product stages and their mutants
    nfft_stage = refs[-1]["stages"][0]
    _check_stage("stft", np.concatenate([r["stages"][0][1] for r in refs]), nfft_stage[2],
                 np.concatenate([r["stages"][0][3] for r in refs]), np.concatenate([r["stages"][0][4] for r in refs]), c.n_fft)
    _check_stage("mel", np.concatenate([r["stages"][1][1] for r in refs]), refs[-1]["stages"][1][2],
                 np.concatenate([r["stages"][1][3] for r in refs]), np.concatenate([r["stages"][1][4] for r in refs]),
                 1 + c.n_fft // 2)
    nb = 1 + c.n_fft // 2
    for ui, (w, r) in enumerate(zip(wavs, refs)):
        if r["frames"] == 0:
            continue
        A32 = r["stages"][0][1].astype(np.float32)
        reim = A32 @ r["stages"][0][2].astype(np.float32)
        re, im = reim[:, :nb], reim[:, nb:]
        mag = np.sqrt(re * re + im * im)
        mel = mag @ basis.T
        lg = np.log10(np.maximum(mel, np.float32(1e-10)))
        assert lg.dtype == np.float32
        assert fb.ratio(reim, r["reim"], r["b_reim"]) <= 1.0
        assert fb.ratio(mag, r["spec"], r["b_spec"]) <= 1.0
        assert fb.ratio(mel, r["mel"], r["b_mel"]) <= 1.0
        assert fb.ratio(lg, r["log10"], r["b_log10"], r["usable"]) <= 1.0
        assert (~r["usable"]).mean() < 0.01
        if ui == 1:                                          # the all-zero utterance
            assert np.array_equal(lg, np.full_like(lg, lg[0, 0])) and r["usable"].all() and not r["b_mel"].any()
        elif c.n_fft >= 400:
            # one bin of one frame off by one percent: the magnitude bound must see it
            wrong = r["spec"].copy()
            f0, k0 = wrong.shape[0] // 2, int(np.argmax(wrong[wrong.shape[0] // 2]))
            wrong[f0, k0] *= 1.01
            assert fb.ratio(wrong, r["spec"], r["b_spec"]) > 1.0


def test_sinusoid_bound_accepts_the_fp32_formula_and_rejects_a_shifted_table():
    for size, npos, start, omega in sc.SIN_CASES:
        want, bound = sc.sinusoid_reference(npos, size, omega, start)
        ch = np.arange(0, size, 2, dtype=np.float32)
        idx = np.arange(start, start + npos, dtype=np.float32)
        p = (idx[:, None] * np.float32(omega)) / np.power(np.float32(10000.0), ch / np.float32(size))
        got = np.zeros((npos, size), np.float32)
        got[:, 0::2], got[:, 1::2] = np.sin(p), np.cos(p)
        assert p.dtype == np.float32 and fb.ratio(got, want, bound) <= 1.0
        off, _ = sc.sinusoid_reference(npos, size, omega, start + 1)         # positions off by one
        assert fb.ratio(off, want, bound) > 1.0


def test_sweeps_cover_what_they_promise():
    a = sc.ATT_CASES
    for m in sc.ATT_MASKS:
        for axis, vals in (("Tk", sc.ATT_TK), ("d", sc.ATT_D), ("dv", sc.ATT_DV), ("rows", tuple(sc.ATT_ROWS))):
            assert {getattr(c, axis) for c in a if c.mask == m} == set(vals), (axis, m)
    assert {(c.Tk, c.d) for c in a} == set(itertools.product(sc.ATT_TK, sc.ATT_D))
    assert {(c.Tk, c.dv) for c in a} == set(itertools.product(sc.ATT_TK, sc.ATT_DV))
    assert sc.ATT_LDS_EDGE.d + sc.ATT_LDS_EDGE.Tk == 4096
    cv = sc.CONV_CASES
    assert {(c.Cout, c.k) for c in cv} == set(itertools.product(sc.CONV_COUT, sc.CONV_K))
    assert {c.Cin for c in cv} == set(sc.CONV_CIN) and {c.B for c in cv} == {1, 3}
    for k in sc.CONV_K:
        want = {(p, t) for p in sc.conv_pads(k) for t in sc.conv_ts(k) if t + 2 * p - k + 1 >= 1}
        assert {(c.pad, c.T) for c in cv if c.k == k} == want
        assert {k, k + 2} <= {c.pad for c in cv if c.k == k and c.B == 3}
    assert {(c.bias, c.bn) for c in cv} == set(itertools.product((False, True), repeat=2))
    assert {c.layout for c in cv} == {"NCL", "NLC"}
    mm = sc.MM_CASES
    assert {(c.M, c.N) for c in mm} == set(itertools.product(sc.MM_M, sc.MM_N))
    assert {(c.K, c.N, c.bias) for c in mm} == set(itertools.product(sc.MM_K, sc.MM_N, (False, True)))
    assert {c.B * c.Cout for c in sc.CELL_CASES} == {1, 5, 8, 129}
    assert {(c.Cin, c.k, c.dil) for c in sc.CELL_CASES} == {(64, 3, 1), (80, 2, 7), (5, 9, 3), (128, 1, 1)}
    assert {128, 129} <= {c.total_frames for c in sc.MEL_CFGS}
    assert math.isclose(fb.U, np.finfo(np.float32).eps / 2)
