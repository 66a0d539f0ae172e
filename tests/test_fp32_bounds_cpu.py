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


@pytest.mark.parametrize("c", sc.GEMM_CASES + sc.GEMM_TAIL_CASES, ids=sc.gemm_id)
def test_split_gemm_bounds(c):
    """the split bound accepts the numpy emulation of the algorithm (block scale, float16 hi / lo, three products, float32
    accumulation) and rejects the three standing mutants and the split kernel's own, for every case"""
    p = sc.gemm_problem(c)
    ref = sc.gemm_reference(p)
    A, W, y, b = ref["Aim"], ref["Wim"], ref["pre"], ref["b_pre"]
    emu = fb.split_emulation(A, W, ref["sa"], ref["sw"])
    if c.bias:
        emu = emu + p["bias"]
    assert emu.dtype == np.float32 and fb.ratio(emu, y, b) <= 1.0
    for name, wrong in {**fb.mutants(A, W, y), **fb.split_mutants(A, W, y, slab=p["loud"])}.items():
        assert fb.ratio(wrong, y, b) > 1.0, f"the bound accepts the '{name}' mutant"
    if c.taps > 1 and c.M > 8:
        # (b) a row scaled by its own maximum, next to a neighbour 2^12 larger: its taps' values overflow fp16
        A2 = p["A"].copy()
        A2[1::2] *= np.float32(2.0 ** 12)
        p2 = dict(p, A=A2)
        r2 = sc.gemm_reference(p2)
        _, _, _, _, own = sc.gemm_operands(p2)
        wrong = fb.split_mutants(r2["Aim"], r2["Wim"], r2["pre"], fb.act_scale(own)[:, None], r2["sw"], r2["sa"])["ownscale"]
        assert fb.ratio(wrong, r2["pre"] - (p["bias"] if c.bias else 0), r2["b_pre"]) > 1.0
        emu2 = fb.split_emulation(r2["Aim"], r2["Wim"], r2["sa"], r2["sw"]) + (p["bias"] if c.bias else np.float32(0))
        assert fb.ratio(emu2, r2["pre"], r2["b_pre"]) <= 1.0
    if c.res and c.gaps:
        # (c) a gap row that keeps its residual
        gaps = sc.gemm_gap_rows(c.M)
        for name, wrong in fb.gemm_epilogue_mutants(ref["C"], p["res"][:, :c.N], gaps).items():
            assert fb.ratio(wrong, ref["C"], ref["b_C"]) > 1.0, name


@pytest.mark.parametrize("c", sc.ROW_CASES, ids=sc.row_id)
def test_rowgemm_plain_bounds(c):
    x, w, b = sc.rowgemm_inputs(c.M, c.K, c.N, bias=c.bias)
    want, _ = sc.matmul_reference(x, w, b)
    A, W = x.astype(np.float64), w.astype(np.float64)
    _check_stage("rowgemm", A, W, want, np.abs(A) @ np.abs(W), c.K, None if b is None else b.astype(np.float64))


@pytest.mark.parametrize("K", sc.ROW_LN_K)
def test_rowgemm_layernorm_bounds(K):
    M, N = 31, 80
    _, w, bias = sc.rowgemm_inputs(M, K, N, "lnw")
    x, g, beta = sc.layernorm_rows(M, K)
    want, bound, xn, b_xn = sc.rowgemm_ln_reference(x, g, beta, w, bias)
    mean = x.sum(1, keepdims=True, dtype=np.float32) * np.float32(1.0 / K)
    d = x - mean
    rstd = np.float32(1.0) / np.sqrt((d * d).sum(1, keepdims=True, dtype=np.float32) * np.float32(1.0 / K) + np.float32(1e-5))
    xn32 = d * rstd * g + beta
    assert xn32.dtype == np.float32 and fb.ratio(xn32, xn, b_xn) <= 1.0
    assert np.all(xn32[0] == beta) or fb.ratio(xn32[:1], xn[:1], b_xn[:1]) <= 1.0      # the constant row
    assert fb.ratio(xn32 @ w + bias, want, bound) <= 1.0
    for name, wrong in fb.mutants(xn, w.astype(np.float64), want).items():
        assert fb.ratio(wrong, want, bound) > 1.0, name
    # a prologue that divides by K + 1, or forgets eps (the constant row: 0 / 0), must be seen
    assert fb.ratio(xn * np.sqrt((K + 1.0) / K), xn, b_xn) > 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        d64 = x.astype(np.float64) - x.astype(np.float64).mean(1, keepdims=True)
        no_eps = d64 / np.sqrt((d64 * d64).mean(1, keepdims=True)) * g + beta
    assert fb.ratio(no_eps[:1], xn[:1], b_xn[:1]) > 1.0


@pytest.mark.parametrize("H", sc.ROW_LSTM_H)
def test_rowgemm_lstm_bounds(H):
    M, K = 31, 64
    r = sc.rng_for("lstm", H)
    _, w, bias = sc.rowgemm_inputs(M, K, 4 * H, "lstmw")
    x = sc.f32(r.normal(0.3, 1, (M, K)))
    c0 = sc.f32(r.normal(0.2, 1, (M, H)))
    cn, h, b_c, b_h = sc.lstm_reference(x, w, bias, c0.astype(np.float64))
    pre = x @ w + bias
    sig = lambda v: np.float32(1) / (np.float32(1) + np.exp(-v))
    c32 = sig(pre[:, H:2 * H]) * c0 + sig(pre[:, :H]) * np.tanh(pre[:, 2 * H:3 * H])
    h32 = sig(pre[:, 3 * H:]) * np.tanh(c32)
    assert h32.dtype == np.float32 and fb.ratio(c32, cn, b_c) <= 1.0 and fb.ratio(h32, h, b_h) <= 1.0
    # (e) the i and f gate columns of the units swapped
    cw, hw, _, _ = sc.lstm_reference(x, fb.lstm_swap_mutant(w, H), fb.lstm_swap_mutant(bias[None], H)[0], c0.astype(np.float64))
    assert fb.ratio(cw, cn, b_c) > 1.0 and fb.ratio(hw, h, b_h) > 1.0
    for name, wrong in fb.mutants(x, w, pre.astype(np.float64)).items():               # through the cell: one gate of one unit
        cm, hm, _, _ = fb.lstm_bound(wrong[:, :H], wrong[:, H:2 * H], wrong[:, 2 * H:3 * H], wrong[:, 3 * H:], 0.0, c0.astype(np.float64), 0.0)
        assert max(fb.ratio(cm, cn, b_c), fb.ratio(hm, h, b_h)) > 1.0, name


def _through_epilogue(p, ref, pre):
    """largest error / bound of the outputs the epilogue makes of a product `pre`"""
    e = sc.gemm_epilogue_reference(p, pre, np.zeros_like(ref["b_pre"]))
    r = fb.ratio(e["C"], ref["C"], ref["b_C"])
    return max(r, fb.ratio(e["C2"], ref["C2"], ref["b_C2"])) if "C2" in e else r


@pytest.mark.parametrize("name,build", sc.GEMM_FEATURE_PROBLEMS, ids=[n for n, _ in sc.GEMM_FEATURE_PROBLEMS])
def test_gemm_feature_problem_bounds(name, build):
    """the problems of the feature tests of tests/test_gemm_sweep_gpu.py (gate, projection, nsplit, A2, skipped tap, mixed
    magnitudes, given row maxima): what the epilogue makes of the emulated split product is inside the bound of the
    OUTPUT, what it makes of every mutant is outside.  A mutant that touches gap rows only cannot show in the output (a
    gap row is zero whatever the product was) and must be outside the bound of the product."""
    p = build()
    ref = sc.gemm_reference(p)
    A, W, y, b = ref["Aim"], ref["Wim"], ref["pre"], ref["b_pre"]
    emu = fb.split_emulation(A, W, ref["sa"], ref["sw"])
    if p.get("bias") is not None:
        emu = emu + p["bias"]
    assert emu.dtype == np.float32 and fb.ratio(emu, y, b) <= 1.0
    assert _through_epilogue(p, ref, emu.astype(np.float64)) <= 1.0
    gap = np.zeros(p["M"], bool) if p.get("rowvalid") is None else p["rowvalid"] < 0
    for mname, wrong in {**fb.mutants(A, W, y), **fb.split_mutants(A, W, y, slab=p["loud"])}.items():
        assert fb.ratio(wrong, y, b) > 1.0, f"the product bound accepts the '{mname}' mutant"
        if not gap[np.any(wrong != y, axis=1)].all():
            assert _through_epilogue(p, ref, wrong) > 1.0, f"the output bound accepts the '{mname}' mutant"
    if p.get("acc2"):           # (d) C2 overwritten where acc2 asks for +=
        over = sc.gemm_epilogue_reference(p, y, b, acc2=0)["C2"]
        assert fb.ratio(over, ref["C2"], ref["b_C2"]) > 1.0
    if p.get("res") is not None and gap.any() and p.get("epi", 0) == 0:      # (c) a gap row keeps its residual
        for mname, wrong in fb.gemm_epilogue_mutants(ref["C"], p["res"][:, :ref["C"].shape[1]], np.flatnonzero(gap)).items():
            assert fb.ratio(wrong, ref["C"], ref["b_C"]) > 1.0, mname
    if name == "skipped-tap":   # a kernel that ignored tap_w and took the weight rows of tap t for the t-th tap
        q = dict(p, tap_w=[0, 1, 2, 3])
        assert fb.ratio(sc.gemm_reference(q)["C"], ref["C"], ref["b_C"]) > 1.0


def test_rowgemm_dropout_and_stop_head_bounds():
    from oracle import philox_ref
    M, K, N = 31, 64, 80
    x, w, bias = sc.rowgemm_inputs(M, K, N, "drop")
    pre, b = sc.matmul_reference(x, w, bias)
    A, W = x.astype(np.float64), w.astype(np.float64)
    _check_stage("dropout", A, W, pre, np.abs(A) @ np.abs(W), K, bias.astype(np.float64))
    idx = np.arange(N, dtype=np.uint64)
    keep, shifted = philox_ref.dropout_keep(idx, 0.25, 7), philox_ref.dropout_keep(idx + np.uint64(1), 0.25, 7)
    want = np.where(keep, np.maximum(pre, 0) * (1 / 0.75), 0.0)
    bound = fb.epilogue_step(np.maximum(pre, 0) / 0.75, b / 0.75)
    y32 = np.where(keep, np.maximum(x @ w + bias, 0) * np.float32(1 / 0.75), np.float32(0))
    assert y32.dtype == np.float32 and fb.ratio(y32, want, bound) <= 1.0
    assert fb.ratio(np.where(shifted, np.maximum(pre, 0) / 0.75, 0.0), want, bound) > 1.0     # the mask of the next element
    # the stop head: a dot product with one column; its bound must see a dropped product
    for ln in (False, True):
        x6, sw, g, beta = sc.stop_inputs(ln)
        logit, b_logit, xn = sc.stop_reference(x6, sw, g, beta, 0.0)
        s32 = (xn.astype(np.float32) @ sw)
        assert fb.ratio(s32, logit, b_logit) <= 1.0
        for mname, wrong in fb.mutants(xn, sw[:, None].astype(np.float64), logit[:, None]).items():
            assert fb.ratio(wrong[:, 0], logit, b_logit) > 1.0, mname
        assert np.all(np.abs(logit) > 100 * b_logit) and (logit > 0).sum() == 3


def test_split_bound_floor_and_scales():
    """act_scale / weight_scale restate blk_scale_exp / pk_weight_scale_exp: block maximum to [2^13, 2^14), clamps included"""
    for v in (1.0, 0.7, 3e-9, 2.0 ** -41, 1e30, 0.0):
        s = float(fb.act_scale(np.float32(v)))
        if 2.0 ** -40 <= v < 2.0 ** 74:
            assert 2.0 ** 13 <= v * s < 2.0 ** 14
    assert float(fb.act_scale(np.float32(0.0))) == float(fb.act_scale(np.float32(2.0 ** -41))) == 2.0 ** 53
    for v in (1.0, 0.3, 17.0):
        assert 2.0 ** 13 <= v * float(fb.weight_scale(v)) < 2.0 ** 14
    assert float(fb.weight_scale(0.0)) == 1.0 and float(fb.weight_scale(2.0 ** -60)) == 2.0 ** 40


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
    g = sc.GEMM_CASES
    for rp in sc.GEMM_RES_POS:
        sel = [c for c in g if c.res_pos == rp]
        assert {c.M for c in sel} == set(sc.GEMM_M) and {c.N for c in sel} == set(sc.GEMM_N), rp
        assert {(c.Cin, c.taps) for c in sel} == {(k[0], k[1]) for k in sc.GEMM_KSHAPES}
        assert {c.pad for c in sel if c.taps == 5} == {0, 2, 4} and {c.pad for c in sel if c.taps == 3} == {0, 1, 2}
        assert {c.act for c in sel} == {0, 1, 2} and {c.affine for c in sel} == {False, True}
    assert {(c.M, c.N) for c in g} >= set(itertools.product(sc.GEMM_M, sc.GEMM_N))
    assert {(c.K, c.N) for c in sc.ROW_CASES} == set(itertools.product(sc.ROW_K, sc.ROW_N))
    assert {c.M for c in sc.ROW_CASES} == set(sc.ROW_M)
    assert {(c.taps, c.loud) for c in sc.GEMM_TAIL_CASES} == {(ns, sl) for ns in (4, 5, 6, 7) for sl in range(ns)}
    assert {5, 6} <= {c.taps * c.Cin // 32 for c in g} and all(c.taps * c.Cin >= 128 for c in g)
    assert math.isclose(fb.U, np.finfo(np.float32).eps / 2)
