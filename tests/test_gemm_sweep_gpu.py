"""The split-fp16 implicit-conv GEMM (k_gemm_h3<1>, k_gemm_h3<2>, k_row_amax; csrc/gemm.hip) at its own edges, through
pk_op_gemm / pk_op_row_amax, against the fp64 restatement and the derived bounds of tests/sweep_cases.py /
tests/fp32_bounds.py (tests/test_fp32_bounds_cpu.py shows on the host that those bounds reject wrong kernels on these very
inputs).  Every case runs with 64-row tiles, with 128-row tiles and with the launcher's own choice, which must equal one of
the two bit for bit.  ``SWEEP-RATIO`` lines as in tests/test_ops_sweep_gpu.py.
"""
import numpy as np
import pytest
import torch

import fp32_bounds as fb
import sweep_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7777.25)
TILES = {64: "h3-64", 128: "h3-128"}


def _report(test, case, **ratios):
    for name, r in ratios.items():
        print(f"SWEEP-RATIO {test} {case} {name} {r:.4g}")
    return max(ratios.values())


def _run(p, tile=0, math=1, ldc_extra=2, **over):
    """pk_op_gemm on problem p -> (C (rows, ldc) numpy, C2 or None, kernel name); outputs are pre-filled with SENTINEL"""
    from parakeet_amd import engine_ops as eo
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    q = {k: v for k, v in dict(p, **over).items() if k not in ("C2_old", "loud")}
    ncols = q["N"] // 2 if q.get("epi") == 1 else (q["nsplit"] if q.get("nsplit") else (128 if q.get("epi") == 2 else q["N"]))
    ldc = ncols + ldc_extra
    C = torch.full((q["M"] + 1, ldc), float(SENTINEL), device=ctx.device)
    C2 = None
    if q.get("nsplit"):
        n2 = q["N"] - q["nsplit"]
        C2 = torch.full((q["M"] + 1, n2 + 1), float(SENTINEL), device=ctx.device)
        if "C2_old" in p:
            C2[:q["M"], :n2] = ctx.to_device(p["C2_old"])
        q["ldc2"] = n2 + 1
    ran = eo.gemm(C=C, C2=C2, ldc=ldc, math=math, tile=tile, **q)
    return C.cpu().numpy(), None if C2 is None else C2.cpu().numpy(), ran


def _expected(p, ref):
    """(want, bound, stored mask) of the (M + 1, N) visible part of C after out_rowmap"""
    M, N = ref["C"].shape
    want, bound, stored = np.zeros((M + 1, N)), np.zeros((M + 1, N)), np.zeros((M + 1, N), bool)
    rm = p.get("out_rowmap")
    dst = np.arange(M) if rm is None else rm
    ok = dst >= 0
    want[dst[ok]], bound[dst[ok]], stored[dst[ok]] = ref["C"][ok], ref["b_C"][ok], True
    return want, bound, stored


def _check(p, ref, C):
    want, bound, stored = _expected(p, ref)
    N = want.shape[1]
    assert np.all(C[:, N:] == SENTINEL), "columns >= N were written"
    assert np.all(C[:, :N][~stored] == SENTINEL), "an unmapped row or a row >= M was written"
    return fb.ratio(C[:, :N], want, bound, stored)


def _both_tiles(test, cid, p, ref, **over):
    """run at 64- and 128-row tiles: each reports its kernel and is within bound, and the two are bit-equal -> (C, C2)"""
    got = {}
    for tile in (64, 128):
        C, C2, ran = _run(p, tile, **over)
        assert ran == TILES[tile]
        ratios = {f"tile{tile}": _check(p, ref, C)}
        if C2 is not None:
            n2 = ref["C2"].shape[1]
            assert np.all(C2[p["M"]:] == SENTINEL) and np.all(C2[:, n2:] == SENTINEL)
            ratios[f"C2-tile{tile}"] = fb.ratio(C2[:p["M"], :n2], ref["C2"], ref["b_C2"])
        assert _report(test, cid, **ratios) <= 1.0
        got[tile] = (C, C2)
    assert np.array_equal(got[64][0], got[128][0]) and (got[64][1] is None or np.array_equal(got[64][1], got[128][1]))
    return got[64]


@pytest.mark.parametrize("c", sc.GEMM_CASES + sc.GEMM_TAIL_CASES, ids=sc.gemm_id)
def test_split_gemm_sweep(c):
    p = sc.gemm_problem(c)
    ref = sc.gemm_reference(p)
    C, _ = _both_tiles("split_gemm", sc.gemm_id(c), p, ref)
    auto, _, _ = _run(p, 0)
    assert np.array_equal(auto, C)
    gaps = sc.gemm_gap_rows(c.M) if c.gaps else []
    if gaps and not c.rowmap:
        # a gap row holds what the formula in pk_gemm.h says for its res_pos: cshift under AFTER_ACT with an affine, else 0
        want = p["cshift"] if (c.affine and c.res_pos == 0) else np.zeros(c.N, np.float32)
        assert np.array_equal(C[gaps, :c.N], np.broadcast_to(want, (len(gaps), c.N)))


def test_k_threshold_between_the_fp32_and_the_split_kernel():
    for K, kernel in ((96, "fp32"), (128, "h3")):
        r = sc.rng_for("kthr", K)
        p = dict(M=65, N=129, Cin=K, taps=1, pad=0, lda=K, A=sc.f32(r.normal(0.5, 1, (65, K))),
                 W=sc.f32(r.normal(0.3, 1, (K, 129)) / np.sqrt(K)), bias=sc.f32(r.normal(0.2, 0.5, 129)))
        ref = sc.gemm_reference(p, split=kernel == "h3")
        C, _, ran = _run(p, 0)
        assert ran.startswith(kernel), (K, ran)
        assert _report("k_threshold", f"K{K}", y=_check(p, ref, C)) <= 1.0


@pytest.mark.parametrize("taps", (1, 3, 5))
@pytest.mark.parametrize("tile", (64, 128))
def test_block_scaling_is_exact_in_powers_of_two(taps, tile):
    """no bias, no residual: scaling an utterance's rows (one power per utterance, gaps of >= taps zero rows between them;
    per row for taps == 1) or a 128-column block of W by a power of two scales the result by exactly that"""
    r = sc.rng_for("pow2", taps)
    Cin, N, M = 64 if taps > 1 else 160, 300, 200
    A = sc.f32(r.normal(0.5, 1, (M, Cin)))
    if taps == 1:
        rowpow = r.integers(-30, 31, M)
    else:
        rowpow, utt = np.zeros(M, np.int64), 0
        for s in range(0, M, 25):                 # 20 rows of speech, 5 zero rows
            A[s + 20:s + 25] = 0
            rowpow[s:s + 25] = (-30, 30, -7, 12, 0, 30, -30, 3)[utt]
            if s:
                rowpow[s - 2:s] = rowpow[s]       # the last two gap rows' taps reach the NEXT utterance only
            utt += 1
    W = sc.f32(r.normal(0.3, 1, (taps * Cin, N)) / np.sqrt(taps * Cin))
    p = dict(M=M, N=N, Cin=Cin, taps=taps, pad=(taps - 1) // 2, lda=Cin, A=A, W=W)
    base, _, ran = _run(p, tile)
    assert ran == TILES[tile]
    scaled, _, _ = _run(dict(p, A=np.ldexp(A, rowpow[:, None].astype(np.int32))), tile)
    assert np.array_equal(scaled[:M, :N], np.ldexp(base[:M, :N], rowpow[:, None].astype(np.int32)))
    colpow = np.repeat(np.array([9, -20, 20]), 128)[:N].astype(np.int32)   # within the +-40 clamp of the weight exponent
    scaled, _, _ = _run(dict(p, W=np.ldexp(W, colpow[None, :])), tile)
    assert np.array_equal(scaled[:M, :N], np.ldexp(base[:M, :N], colpow[None, :]))


@pytest.mark.parametrize("taps", (3, 5))
def test_mixed_magnitudes_zero_tiles_and_tiny_rows(taps):
    p = sc.mixed_problem(taps)
    ref = sc.gemm_reference(p)
    C, _ = _both_tiles("mixed", f"k{taps}", p, ref)
    N = p["N"]
    assert np.all(np.isfinite(C))
    assert np.all(C[128 + taps:256 - taps, :N] == 0) and np.all(C[100 + taps:110 - taps, :N] == 0)
    assert np.abs(C[302:308, :N]).max() > 0


def test_caller_supplied_row_maxima():
    p = sc.amax_problem(0)
    own, _ = _both_tiles("a_amax", "own", p, sc.gemm_reference(p))
    given, _, _ = _run(dict(p, a_amax=np.abs(p["A"]).max(1).astype(np.float32)), 64)
    assert np.array_equal(own, given)
    p2 = sc.amax_problem(2.0)                     # an upper bound, as producers that know one pass it
    _both_tiles("a_amax", "x2", p2, sc.gemm_reference(p2))


@pytest.mark.parametrize("nsplit,acc2", ((64, 0), (64, 1), (128, 0), (128, 1)))
def test_nsplit_and_the_running_sum(nsplit, acc2):
    p = sc.nsplit_problem(nsplit, acc2)
    ref = sc.gemm_reference(p)
    _, C2 = _both_tiles("nsplit", f"ns{nsplit}-acc{acc2}", p, ref)
    # a gap row of C2 is zeroed, with or without acc2 (gemm.hip, `to2`)
    assert np.all(C2[sc.gemm_gap_rows(p["M"]), :p["N"] - nsplit] == 0)


@pytest.mark.parametrize("N,bias", ((128, False), (128, True), (256, False), (256, True)))
def test_gate_epilogue(N, bias):
    p = sc.gate_problem(N, bias)
    C, _ = _both_tiles("gate", f"N{N}-{'bias' if bias else 'nobias'}", p, sc.gemm_reference(p))
    assert np.all(C[sc.gemm_gap_rows(p["M"]), :N // 2] == 0)


def test_gate_projection_epilogue():
    p = sc.gate_problem(128, True, proj=True)
    C, _ = _both_tiles("gate_proj", "M150", p, sc.gemm_reference(p))
    assert np.all(C[sc.gemm_gap_rows(p["M"]), :128] == 0)


def test_skipped_tap_equals_the_full_convolution_on_zero_rows():
    """tap_w = [0, 1, 3, 4] with the matching offsets skips the middle one of 5 packed taps (4 K slabs): within bound, and
    bit-equal to all 5 taps on the odd output rows, where the skipped tap reads a zero row"""
    full, part = sc.skipped_tap_problem()
    C, _ = _both_tiles("skipped_tap", "k5-tap2", part, sc.gemm_reference(part))
    M, N = part["M"], part["N"]
    for tile in (64, 128):
        f, _, _ = _run(full, tile)
        assert np.array_equal(C[1:M:2, :N], f[1:M:2, :N])
    assert np.all(np.abs(C[1:M - 1:2, :N]).max(1) > 0)


@pytest.mark.parametrize("Cin,Cin2", sc.GEMM_A2_SHAPES)
def test_second_operand_block(Cin, Cin2):
    """4, 7 and 9 K slabs with every kind of slab loud in turn: the first, one in the ring, the first and the last of A2"""
    ns = (3 * Cin + Cin2) // 32
    for loud in sorted({0, ns // 2, 3 * Cin // 32, ns - 1}):
        p = sc.a2_problem(Cin, Cin2, loud)
        _both_tiles("a2", f"Cin{Cin}-Cin2_{Cin2}-loud{loud}", p, sc.gemm_reference(p))
    if (Cin, Cin2) == (64, 32):                   # the same through taps / pad, as the models' plain convolutions are given
        p = sc.a2_problem(Cin, Cin2, 6, explicit=False)
        C, _ = _both_tiles("a2", "tapspad", p, sc.gemm_reference(p))
        E, _, _ = _run(sc.a2_problem(Cin, Cin2, 6), 64)
        assert np.array_equal(C, E)


def test_status_codes():
    r = sc.rng_for("status")
    def prob(Cin=64, taps=3, N=128, **kw):
        return dict(dict(M=8, N=N, Cin=Cin, taps=taps, pad=0, lda=Cin, A=sc.f32(r.normal(size=(8, Cin))),
                         W=sc.f32(r.normal(size=(taps * Cin, N)))), **kw)
    with pytest.raises(NotImplementedError):
        _run(prob(Cin=24))
    with pytest.raises(NotImplementedError):
        _run(prob(taps=13, Cin=16))
    with pytest.raises(NotImplementedError):      # a tap offset that is no whole number of rows, split kernel
        _run(prob(ntaps=3, wtaps=3, tap_off=[0, 64, 100], tap_w=[0, 1, 2]))
    w2 = sc.f32(r.normal(size=(64, 128)))
    with pytest.raises(NotImplementedError):
        _run(prob(epi=2, W2=w2), math=0)
    with pytest.raises(NotImplementedError):
        _run(prob(epi=2, W2=w2, N=256))
    with pytest.raises(ValueError):
        _run(prob(), tile=96)


@pytest.mark.parametrize("C_", (16, 64, 65, 128, 129, 384, 7))
def test_row_amax_is_exact(C_):
    from parakeet_amd import engine_ops as eo
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    r = sc.rng_for("amax", C_)
    lda, margin = C_ + 5, 3
    for nrows in (1, 3, 70):                      # row counts that do not fill a wave, and more than one workgroup
        A = sc.f32(r.normal(0, 1, (margin + nrows + 2, lda)) * np.exp2(r.integers(-20, 20, (margin + nrows + 2, 1))))
        A[:, C_:] = 1e30                          # beyond C: must not be read into the maximum
        dA = ctx.to_device(A)
        out = torch.full((margin + nrows + 2,), float(SENTINEL), device=ctx.device)
        eo.row_amax(dA, lda, C_, -margin, nrows, out, base_row=margin, amax_base=margin)
        got = out.cpu().numpy()
        assert np.array_equal(got[:margin + nrows], np.abs(A[:margin + nrows, :C_]).max(1))
        assert np.all(got[margin + nrows:] == SENTINEL)
