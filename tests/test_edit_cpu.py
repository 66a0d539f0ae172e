"""The numpy restatement of the edit distance and its alignment (tests/edit_ref.py, csrc/pk_edit.h) against the
reference's recorded results (tests/golden/error_rate.json), against brute force over every alignment of tiny pairs, and the
host-side pieces of ``parakeet_amd.utils.error_rate`` and of the two recipes (no GPU)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import edit_ref as er  # noqa: E402


def _golden():
    with open(os.path.join(HERE, "golden", "error_rate.json"), "rt", encoding="utf-8") as f:
        return json.load(f)["cases"]


def _tokens(case):
    from parakeet_amd.utils import error_rate as E
    kw = case["kwargs"]
    if case["fn"] in ("word_errors", "wer"):
        split = lambda s: E.split_words(s, kw.get("ignore_case", False), kw.get("delimiter", " "))   # noqa: E731
    else:
        split = lambda s: E.split_chars(s, kw.get("ignore_case", False), kw.get("remove_space", False))   # noqa: E731
    return split(case["reference"]), split(case["hypothesis"])


def test_golden_covers_what_it_should():
    cases = _golden()
    lens = {len(_tokens(c)[0]) for c in cases}
    assert {0, 1, 63, 64, 65} <= lens and any(125 <= n <= 135 for n in lens)
    assert {c["fn"] for c in cases} == {"word_errors", "char_errors", "wer", "cer"}
    errors = {c["error"] for c in cases if "error" in c}
    assert errors == {"Reference's word number should be greater than 0.", "Length of reference should be greater than 0."}
    assert any(c["kwargs"].get("ignore_case") for c in cases) and any(c["kwargs"].get("remove_space") for c in cases)
    assert any(c["kwargs"].get("delimiter", " ") != " " for c in cases)
    assert any(c["reference"] == c["hypothesis"] != "" for c in cases) and any(c["hypothesis"] == "" != c["reference"] for c in cases)


def test_restatement_and_encode_equal_the_golden():
    from parakeet_amd.utils.error_rate import encode
    cases = _golden()
    toks = [_tokens(c) for c in cases]
    r, h, rl, hl = encode([t[0] for t in toks], [t[1] for t in toks])          # one vocabulary for all cases
    assert r.dtype == h.dtype == rl.dtype == hl.dtype == np.int32 and r.size == rl.sum() and h.size == hl.sum()
    ro, ho = np.concatenate(([0], np.cumsum(rl))), np.concatenate(([0], np.cumsum(hl)))
    for b, c in enumerate(cases):
        d = er.distance(r[ro[b]:ro[b + 1]], h[ho[b]:ho[b + 1]])
        if "error" in c:
            assert rl[b] == 0
        elif isinstance(c["result"], list):
            assert [float(d), int(rl[b])] == c["result"], (b, c["fn"])
        else:
            assert float(d) / int(rl[b]) == c["result"], (b, c["fn"])


def test_encode():
    from parakeet_amd.utils.error_rate import encode
    r, h, rl, hl = encode([["ab", "c", "ab", "天"], [], ["x"]], [["c", "ab"], ["天", "ab", "zz"], []])
    assert rl.tolist() == [4, 0, 1] and hl.tolist() == [2, 3, 0]
    assert r.tolist() == [-1, ord("c"), -1, ord("天"), ord("x")] and h.tolist() == [ord("c"), -1, ord("天"), -1, -2]
    r, h, rl, hl = encode([], [])
    assert r.size == h.size == rl.size == hl.size == 0 and r.dtype == np.int32
    with pytest.raises(ValueError, match="1 references, 2 hypotheses"):
        encode([["a"]], [["a"], ["b"]])


_shapes = {}


def _all_shapes(N, M):
    """Every monotone alignment of an N x M pair, whatever its ids: (gaps (A,), diagonal cells (A, N * M) 0 / 1) over the A
    alignments ``edit_ref.all_alignments`` enumerates.  An alignment's cost is its gaps plus the unequal cells on its diagonal
    steps."""
    if (N, M) not in _shapes:
        alls = er.all_alignments(list(range(N)), [-1 - j for j in range(M)])          # no equal ids: diagonal steps are SUB
        gaps = np.array([sum(op != er.SUB for op in a) for a in alls], dtype=np.int64)
        diag = np.zeros((len(alls), max(N * M, 1)), dtype=np.int64)
        for k, a in enumerate(alls):
            ri, hi = er.index_pairs(a)
            for op, i, j in zip(a, ri, hi):
                if op == er.SUB:
                    diag[k, i * M + j] = 1
        _shapes[N, M] = (gaps, diag)
    return _shapes[N, M]


def _brute_costs(ref, hyp):
    """The cost of every alignment of the pair."""
    N, M = len(ref), len(hyp)
    gaps, diag = _all_shapes(N, M)
    differ = np.zeros(max(N * M, 1), dtype=np.int64)
    if N * M:
        differ[:] = (np.asarray(ref)[:, None] != np.asarray(hyp)[None, :]).reshape(-1)
    return gaps + diag @ differ


def _brute_table(ref, hyp):
    N, M = len(ref), len(hyp)
    D = np.zeros((N + 1, M + 1), dtype=np.int64)
    for i in range(N + 1):
        for j in range(M + 1):
            D[i, j] = _brute_costs(ref[:i], hyp[:j]).min()
    return D


def test_brute_force_enumeration_itself():
    ref, hyp = [0, 1, 1], [1, 0]
    alls = er.all_alignments(ref, hyp)
    assert len(alls) == len(set(alls)) == 25                       # the Delannoy number D(3, 2)
    assert sorted(er.cost(a) for a in alls) == sorted(_brute_costs(ref, hyp).tolist())
    assert len(_all_shapes(5, 5)[0]) == 1683


def test_restatement_against_brute_force():
    """Every pair with N, M <= 5 over 2 symbols: the distance is the minimum over all alignments, the ops are a minimiser and
    the one the tie rule picks on the brute-force table; the three identities."""
    ties = pairs = 0
    for N in range(6):
        for M in range(6):
            for code in range(2 ** (N + M)):
                ref = [(code >> k) & 1 for k in range(N)]
                hyp = [(code >> (N + k)) & 1 for k in range(M)]
                got = er.align(ref, hyp)
                costs = _brute_costs(ref, hyp)
                assert got["distance"] == costs.min(), (ref, hyp)
                # the ops are an alignment of the pair (hits on equal ids, substitutions on unequal ones) of that cost
                ops = got["ops"]
                ri, hi = er.index_pairs(ops)
                assert ri[ri >= 0].tolist() == list(range(N)) and hi[hi >= 0].tolist() == list(range(M))
                assert all((ref[i] == hyp[j]) == (op == er.HIT) for op, i, j in zip(ops, ri, hi) if op in (er.HIT, er.SUB))
                assert er.cost(ops) == costs.min()
                D = _brute_table(ref, hyp)
                assert np.array_equal(D, er.table(ref, hyp))
                assert np.array_equal(ops, er.walk(ref, hyp, D)), (ref, hyp)
                H, S, Dl, I = got["counts"].tolist()
                assert S + Dl + I == got["distance"] and H + S + Dl == N and H + S + I == M
                assert max(N, M) <= got["length"] <= N + M
                ties += int((costs == costs.min()).sum() > 1)
                pairs += 1
    assert pairs == 63 * 63 and ties > 1000                        # the tie rule was exercised


def test_fast_table_equals_the_definition():
    rng = np.random.default_rng(5)
    for _ in range(60):
        N, M, A = int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(1, 5))
        ref, hyp = rng.integers(A, size=N), rng.integers(A, size=M)
        assert np.array_equal(er.table(ref, hyp), er.table_slow(ref.tolist(), hyp.tolist()))
        a, b = er.align(ref, hyp), er.align(ref, hyp, slow=True)
        assert a["distance"] == b["distance"] and np.array_equal(a["ops"], b["ops"])
        H, S, D, I = a["counts"].tolist()
        assert S + D + I == a["distance"] and H + S + D == N and H + S + I == M
        ri, hi = er.index_pairs(a["ops"])
        assert ri[ri >= 0].tolist() == list(range(N)) and hi[hi >= 0].tolist() == list(range(M))
        assert all(ref[i] == hyp[j] for op, i, j in zip(a["ops"], ri, hi) if op == er.HIT)
        assert all(ref[i] != hyp[j] for op, i, j in zip(a["ops"], ri, hi) if op == er.SUB)


def test_planted_edits_and_disjoint_alphabets():
    rng = np.random.default_rng(6)
    for n in (0, 1, 30, 200):
        ref = rng.integers(30, size=n).astype(np.int32)
        for k in (0, 1, 5, 40):
            hyp, planted = er.plant(rng, ref, k, 30)
            assert er.distance(ref, hyp) <= planted
        assert er.distance(ref, ref) == 0
    for N, M in ((0, 0), (0, 7), (7, 0), (5, 9), (64, 3)):
        assert er.distance(np.arange(N), 1000 + np.arange(M)) == max(N, M)
        assert er.distance(np.zeros(N, int), np.ones(M, int)) == max(N, M)


def test_the_recipes_cleaning_functions():
    import frontend_g2p_wer as g2p
    import frontend_textnorm_cer as tn
    assert g2p.text_cleaner("卡尔普#2陪外孙#1玩滑梯#4。") == "卡尔普陪外孙玩滑梯。"
    assert g2p.text_cleaner("“他说：（好）……”") == "他说，好，"
    assert g2p.text_cleaner("走吧…。") == "走吧。"
    assert g2p.text_cleaner("甲、乙；丙——丁—戊…") == "甲，乙，丙，丁，戊，"
    assert g2p.text_cleaner("#5 stays") == "#5 stays"
    assert g2p.SILENCE_TOKENS == {"sp", "sil", "sp1", "spl"}
    assert tn.del_en_add_space("你好aBC") == "你 好"
    assert tn.del_en_add_space("aBC") == "" and tn.del_en_add_space("") == ""
    assert tn.del_en_add_space("一a二 三") == "一 二   三"
    assert tn.del_en_add_space("12点") == "1 2 点"


def test_format_confusions():
    import collections
    from parakeet_amd.utils.error_rate import format_confusions
    Conf = collections.namedtuple("Conf", "substitutions deletions insertions")
    c = Conf(collections.Counter({("a", "b"): 2, ("c", "d"): 2, ("e", "f"): 1}), collections.Counter({"x": 3}), collections.Counter())
    assert format_confusions(c, 2) == ["substitutions (5):", "2\ta -> b", "2\tc -> d", "deletions (3):", "3\tx", "insertions (0):"]
