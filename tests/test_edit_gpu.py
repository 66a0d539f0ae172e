"""The edit distance and its alignment on the engine (csrc/edit.hip, csrc/pk_edit.h) against the numpy
restatement tests/edit_ref.py and the reference's recorded results (tests/golden/error_rate.json), through the C ABI, through
``parakeet_amd.alignment`` / ``parakeet_amd.utils.error_rate`` and through the two recipes.

Everything is integer: distance, counts, the number of ops and the ops themselves are compared with ``==``; this file has no
tolerance."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import edit_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 3                      # an id in the gaps and the padding: a symbol of the random kind, a stranger to the others
OPS_SENTINEL = 0xEE
OUT_SENTINEL = -7
_EDGE = (0, 1, 2, 63, 64, 65)
# every strip height's 64 R - 1, 64 R, 64 R + 1 (R = 1 is in _EDGE); 1025 is the first length past a single pass
_STRIPS = tuple(64 * R + d for R in (2, 4, 8, 16) for d in (-1, 0, 1))
SHAPES = [(a, b) for a in _EDGE for b in _EDGE] + sorted({(a, b) for a in _STRIPS for b in (1, 65)} |
                                                         {(b, a) for a in _STRIPS for b in (1, 65)})
SMALL = [i for i, (N, M) in enumerate(SHAPES) if max(N, M) <= 65]
KINDS = ("random", "equal", "disjoint", "planted")
_cache = {}


def _np(t):
    return t.as_subclass(torch.Tensor).detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _ids(N, M, kind, seed):
    """random: 4 symbols, ties everywhere; equal: one symbol; disjoint: no common symbol; planted: hyp is ref (repeated or cut
    to M ids, 30 symbols) with a tenth of M edits planted."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 4, size=N).astype(np.int32), rng.integers(0, 4, size=M).astype(np.int32)
    if kind == "equal":
        return np.full(N, 5, np.int32), np.full(M, 5, np.int32)
    if kind == "disjoint":
        return rng.integers(10, 20, size=N).astype(np.int32), rng.integers(30, 40, size=M).astype(np.int32)
    ref = rng.integers(100, 130, size=N).astype(np.int32)
    base = np.resize(ref, M) if N else rng.integers(100, 130, size=M).astype(np.int32)
    hyp = er.plant(rng, base, max(1, M // 10), 30)[0]
    hyp = np.where(hyp < 100, hyp + 100, hyp)[:M]                  # (planted symbols come from the same 30)
    hyp = np.concatenate([hyp, rng.integers(100, 130, size=M - hyp.size)]).astype(np.int32)
    return ref, hyp


def _case(N, M, kind, seed):
    ref, hyp = _ids(N, M, kind, seed)
    assert ref.size == N and hyp.size == M
    return dict(ref=ref, hyp=hyp, want=er.align(ref, hyp))


def _cases(kind):
    """The shapes' inputs and their restatement results, computed once."""
    if kind not in _cache:
        _cache[kind] = [_case(N, M, kind, 100 * i + 7) for i, (N, M) in enumerate(SHAPES)]
        if kind in ("equal", "disjoint"):
            assert all(k["want"]["distance"] == (abs(N - M) if kind == "equal" else max(N, M)) for k, (N, M) in zip(_cache[kind], SHAPES))
    return _cache[kind]


def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _i64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int64)


def _call(mode, refbuf, hypbuf, offs_r, offs_h, n, m, check=True, null=()):
    """pk_edit_run on flat int32 host buffers -> (0, per-pair dicts) or (status code, message).  Every output starts as a
    sentinel: ops from P on must keep it, and so must everything after a refusal and what mode 0 does not write."""
    from parakeet_amd import _capi
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    flat = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)   # noqa: E731
    tr = ctx.to_device(np.concatenate([flat(refbuf), [SENTINEL]]).astype(np.int32), dtype=torch.int32)
    th = ctx.to_device(np.concatenate([flat(hypbuf), [SENTINEL]]).astype(np.int32), dtype=torch.int32)
    n, m = np.ascontiguousarray(n, dtype=np.int32), np.ascontiguousarray(m, dtype=np.int32)
    offs_r, offs_h = _i64(offs_r), _i64(offs_h)
    B = int(n.size)
    cap = np.maximum(n.astype(np.int64) + m, 0)
    po = np.concatenate(([0], np.cumsum(cap)))
    ops = torch.full((max(int(po[-1]), 1),), OPS_SENTINEL, dtype=torch.uint8, device=ctx.device)
    dist = torch.full((max(B, 1),), OUT_SENTINEL, dtype=torch.int32, device=ctx.device)
    ln = torch.full((max(B, 1),), OUT_SENTINEL, dtype=torch.int32, device=ctx.device)
    counts = torch.full((max(B, 1), 4), OUT_SENTINEL, dtype=torch.int32, device=ctx.device)
    arg = lambda name, t: None if name in null else dptr(t)        # noqa: E731
    rc = ctx.lib.pk_edit_run(ctx.handle, arg("ref", tr), arg("hyp", th), _ptr(offs_r, C.c_int64), _ptr(offs_h, C.c_int64),
                             None if "n" in null else _ptr(n, C.c_int32), _ptr(m, C.c_int32), B, int(mode), arg("dist", dist),
                             arg("counts", counts), arg("ops", ops), arg("len", ln))
    ctx.sync()
    oh, dh, lh, ch = _np(ops), _np(dist), _np(ln), _np(counts)
    if rc != 0:
        assert np.all(oh == OPS_SENTINEL) and np.all(dh == OUT_SENTINEL) and np.all(lh == OUT_SENTINEL) and np.all(ch == OUT_SENTINEL)
        if check:
            _capi.check(rc)
        return rc, ctx.lib.pk_last_error().decode()
    if mode == 0:
        assert np.all(oh == OPS_SENTINEL) and np.all(lh == OUT_SENTINEL) and np.all(ch == OUT_SENTINEL), "mode 0 writes the distance alone"
        return 0, [dict(distance=int(dh[b])) for b in range(B)]
    out = []
    for b in range(B):
        P = int(lh[b])
        assert max(n[b], m[b]) <= P <= cap[b]
        o = oh[po[b]:po[b + 1]]
        assert np.all(o[P:] == OPS_SENTINEL), "entries from P on are never written"
        out.append(dict(distance=int(dh[b]), ops=o[:P], length=P, counts=ch[b]))
    return 0, out


def _pack(arrs, order, gap=3):
    """The arrays in ``order``, each at an offset of its own in one buffer whose every other entry is SENTINEL."""
    offs, o = [], gap
    for i in order:
        offs.append(o)
        o += arrs[i].size + gap
    buf = np.full(o, SENTINEL, dtype=np.int32)
    for i, off in zip(order, offs):
        buf[off:off + arrs[i].size] = arrs[i]
    return buf, offs


def _batch(cases, order, mode, **kw):
    br, o_r = _pack([k["ref"] for k in cases], order)
    bh, o_h = _pack([k["hyp"] for k in cases], order, gap=5)
    return _call(mode, br, bh, o_r, o_h, [cases[i]["ref"].size for i in order], [cases[i]["hyp"].size for i in order], **kw)


def _same(got, want, what, mode=1):
    assert got["distance"] == want["distance"], (what, got["distance"], want["distance"])
    if mode == 1:
        assert got["length"] == want["length"], what
        assert np.array_equal(got["ops"], want["ops"]), what
        assert np.array_equal(got["counts"], want["counts"]), what
        H, S, D, I = (int(v) for v in got["counts"])
        assert S + D + I == got["distance"] and H + S + D + I == got["length"], what


@pytest.mark.parametrize("kind", KINDS)
def test_exact_in_a_ragged_batch_in_two_orders(kind):
    cases = _cases(kind)
    order = list(range(len(SHAPES)))
    for od in (order, order[::-1]):
        for mode in (0, 1):
            _, got = _batch(cases, od, mode)
            for k, i in enumerate(od):
                _same(got[k], cases[i]["want"], (kind, mode, SHAPES[i]), mode)
    for (N, M), k in zip(SHAPES, cases):
        H, S, D, I = k["want"]["counts"].tolist()
        assert H + S + D == N and H + S + I == M
        if kind == "disjoint":
            assert H == 0 and k["want"]["length"] == max(N, M)    # every tie went to the substitution


def test_each_pair_alone_and_contiguous():
    cases = _cases("random")
    for i, k in enumerate(cases):
        for mode in (0, 1):
            _, got = _call(mode, k["ref"], k["hyp"], None, None, [SHAPES[i][0]], [SHAPES[i][1]])
            _same(got[0], k["want"], (mode, SHAPES[i]), mode)
    sub = SMALL[::3]
    for mode in (0, 1):
        _, got = _call(mode, np.concatenate([cases[i]["ref"] for i in sub]), np.concatenate([cases[i]["hyp"] for i in sub]),
                       None, None, [SHAPES[i][0] for i in sub], [SHAPES[i][1] for i in sub])
        for k, i in enumerate(sub):
            _same(got[k], cases[i]["want"], SHAPES[i], mode)


@pytest.mark.parametrize("kind", ["random", "planted"])
def test_padded_tensors_with_sentinel_padding(kind):
    from parakeet_amd.alignment import edit_align, edit_distance
    cases = _cases(kind)
    groups = {}
    for i, (N, M) in enumerate(SHAPES):
        groups.setdefault((N > 65, M > 65), []).append(i)
    assert len(groups) == 3                                        # (no shape is long on both sides)
    for idx in groups.values():
        Nm, Mm = max(SHAPES[i][0] for i in idx) + 2, max(SHAPES[i][1] for i in idx) + 3
        B = len(idx)
        pr, ph = np.full((B, Nm), SENTINEL, np.int32), np.full((B, Mm), SENTINEL, np.int32)
        for k, i in enumerate(idx):
            N, M = SHAPES[i]
            pr[k, :N], ph[k, :M] = cases[i]["ref"], cases[i]["hyp"]
        n, m = [SHAPES[i][0] for i in idx], [SHAPES[i][1] for i in idx]
        for mode in (0, 1):
            _, got = _call(mode, pr, ph, np.arange(B) * Nm, np.arange(B) * Mm, n, m)
            for k, i in enumerate(idx):
                _same(got[k], cases[i]["want"], SHAPES[i], mode)
        # the same through the Python interface: padded tensors with lengths, lists of host arrays
        a = edit_align(torch.from_numpy(pr), torch.from_numpy(ph), n, m)
        b = edit_align([cases[i]["ref"] for i in idx], [cases[i]["hyp"] for i in idx])
        d0 = edit_distance(torch.from_numpy(pr.astype(np.int64)), torch.from_numpy(ph.astype(np.int64)), n, m)
        d1 = edit_distance([cases[i]["ref"].tolist() for i in idx], [torch.from_numpy(cases[i]["hyp"]) for i in idx])
        for k, i in enumerate(idx):
            want = cases[i]["want"]
            for r in (a[k], b[k]):
                assert r.distance == want["distance"] and r.length == want["length"] and list(r.counts) == want["counts"].tolist()
                assert np.array_equal(_np(r.ops), want["ops"]) and _np(r.ops).dtype == np.uint8
                assert (r.ref_len, r.hyp_len) == SHAPES[i]
            assert d0[k] == d1[k] == want["distance"]
    one = edit_align(cases[SMALL[8]]["ref"], cases[SMALL[8]]["hyp"])
    assert np.array_equal(_np(one.ops), cases[SMALL[8]]["want"]["ops"]) and isinstance(one.distance, int)
    assert edit_distance([1, 2, 3], [1, 3]) == 1 and edit_distance([], [4, 4]) == 2 and edit_distance([], []) == 0


@pytest.mark.parametrize("mode", [0, 1])
def test_the_largest_pair(mode):
    if "largest" not in _cache:
        rng = np.random.default_rng(77)
        ref, hyp = rng.integers(0, 2, size=4096).astype(np.int32), rng.integers(0, 2, size=4096).astype(np.int32)
        _cache["largest"] = dict(ref=ref, hyp=hyp, want=er.align(ref, hyp))
    k = _cache["largest"]
    _, got = _call(mode, k["ref"], k["hyp"], None, None, [4096], [4096])
    _same(got[0], k["want"], "4096 x 4096", mode)


def test_both_op_stores_and_several_passes():
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    w = C.c_int32()
    assert ctx.lib.pk_edit_lds_words(C.byref(w)) == 0
    lds = int(w.value)
    assert 1024 <= lds <= 40960

    def words(N, M):                                               # pk_edit.h: M words per strip of R rows
        R = 1
        while R < 16 and 64 * R < N:
            R *= 2
        return M * -(-N // R)
    assert [words(N, 1) for N in (0, 1, 64, 65, 128, 129, 1024, 1025, 4096)] == [0, 1, 64, 33, 64, 33, 64, 65, 256]
    # LDS and global at one pass with 16 and with 1 row per strip; two passes in LDS; two and three passes in the workspace
    shapes = [(1024, lds // 64), (1024, lds // 64 + 1), (64, lds // 64), (64, lds // 64 + 1), (1500, 70), (1025, lds // 65 + 1),
              (2100, lds // 132 + 7)]
    assert [words(N, M) <= lds for N, M in shapes] == [True, False, True, False, True, False, False]
    cases = [_case(N, M, KINDS[k % 4], 900 + k) for k, (N, M) in enumerate(shapes)]
    for mode in (0, 1):
        _, got = _batch(cases, list(range(len(cases))), mode)
        for k in range(len(cases)):
            _same(got[k], cases[k]["want"], shapes[k], mode)
    for k in (1, 3, 5):                                            # the global store alone: the workspace starts at this pair
        _, one = _batch(cases, [k], 1)
        _same(one[0], cases[k]["want"], shapes[k])


def test_envelope_and_argument_refusals_launch_nothing():
    from parakeet_amd.alignment import edit_align, edit_distance
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    tiny = np.zeros(8, np.int32)
    ctx.sync()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        for mode in (0, 1):
            rc, msg = _call(mode, tiny, tiny, None, None, [4097], [2], check=False)
            assert rc == -3 and "4097 ref ids" in msg and "4096" in msg
            rc, msg = _call(mode, tiny, tiny, None, None, [2, 2], [2, 4097], check=False)
            assert rc == -3 and "pair 1 has 4097 hyp ids" in msg
            rc, msg = _call(mode, tiny, tiny, None, None, [2, -1], [2, 1], check=False)
            assert rc == -1 and "pair 1 has a negative length" in msg
            rc, msg = _call(mode, tiny, tiny, None, None, [], [], check=False)
            assert rc == -1 and "batch size" in msg
            rc, msg = _call(mode, tiny, tiny, [0, -4], [0, 2], [2, 2], [2, 2], check=False)
            assert rc == -1 and "pair 1 has a negative offset" in msg
            rc, msg = _call(mode, tiny, tiny, None, None, np.zeros(65536, np.int32), np.zeros(65536, np.int32), check=False)
            assert rc == -3 and "65536 pairs" in msg and "65535" in msg
            for name in ("ref", "hyp", "n", "dist"):
                rc, msg = _call(mode, tiny, tiny, None, None, [2], [2], check=False, null=(name,))
                assert rc == -1 and "NULL" in msg
        for name in ("counts", "ops", "len"):
            rc, msg = _call(1, tiny, tiny, None, None, [2], [2], check=False, null=(name,))
            assert rc == -1 and "NULL" in msg
        rc, msg = _call(2, tiny, tiny, None, None, [2], [2], check=False)
        assert rc == -1 and "mode" in msg
        with pytest.raises(NotImplementedError, match="4097 ref ids"):
            edit_distance(np.zeros(4097, np.int32), [1])
        with pytest.raises(NotImplementedError, match="4096"):
            edit_align([[1]], [np.zeros(5000, np.int32)])
        with pytest.raises(ValueError, match="1 sequences ref, 2 sequences hyp"):
            edit_distance([[1]], [[1], [2]])
        with pytest.raises(ValueError, match="lengths"):
            edit_distance(np.zeros((2, 3), np.int32), np.zeros((2, 3), np.int32), [1, 4], [1, 1])
        with pytest.raises(ValueError, match="integers"):
            edit_distance([0.5, 1.0], [1])
        assert all(c == 0 for k, (c, _) in ctx.prof_dump().items() if k.startswith("edit"))
        k = _case(9, 4, "random", 1)
        _, got = _call(1, k["ref"], k["hyp"], None, None, [9], [4])
        _same(got[0], k["want"], "after the refusals")
        assert ctx.prof_dump()["edit"][0] == 1
    finally:
        ctx.prof_enable(False)


# ------------------------------------------------------------------------------------------------------- the Python surface
def _golden():
    with open(os.path.join(HERE, "golden", "error_rate.json"), "rt", encoding="utf-8") as f:
        return json.load(f)["cases"]


def test_error_rates_equal_the_reference_on_every_golden_case():
    from parakeet_amd.utils import error_rate as E
    import parakeet_amd.utils as U
    assert U.error_rate is E and {"word_errors", "char_errors", "wer", "cer"} <= set(E.__all__)
    cases = _golden()
    for c in cases:
        fn = getattr(E, c["fn"])
        if "error" in c:
            with pytest.raises(ValueError) as e:
                fn(c["reference"], c["hypothesis"], **c["kwargs"])
            assert str(e.value) == c["error"]
            continue
        got = fn(c["reference"], c["hypothesis"], **c["kwargs"])
        if isinstance(c["result"], list):
            assert isinstance(got, tuple) and isinstance(got[0], float) and isinstance(got[1], int)
            assert list(got) == c["result"], c
        else:
            assert isinstance(got, float) and got == c["result"], c
    # the batch functions equal the single calls; the corpus rates are sum of distances / sum of lengths
    for name, batch, corpus in (("word_errors", E.word_errors_batch, E.corpus_wer), ("char_errors", E.char_errors_batch, E.corpus_cer)):
        sub = [c for c in cases if c["fn"] == name and not c["kwargs"]]
        assert len(sub) >= 10
        d, n = batch([c["reference"] for c in sub], [c["hypothesis"] for c in sub])
        assert d.dtype == np.float64 and d.tolist() == [c["result"][0] for c in sub] and n.tolist() == [c["result"][1] for c in sub]
        want = sum(c["result"][0] for c in sub) / sum(c["result"][1] for c in sub)     # how both reference recipes average
        assert corpus([c["reference"] for c in sub], [c["hypothesis"] for c in sub]) == want
    with pytest.raises(ValueError, match="word number"):
        E.corpus_wer(["", " "], ["a", "b"])
    d, n = E.word_errors_batch(["A b", "a|b"], ["a B", "b"], ignore_case=True)
    assert d.tolist() == [0.0, 1.0] and n.tolist() == [2, 1]
    d, n, als = E.token_errors_batch([["x", "y"], []], [["y"], ["z", "z"]], return_alignments=True)
    assert d.tolist() == [1, 2] and n.tolist() == [2, 0] and [a.counts.deletions for a in als] == [1, 0]


def test_index_pairs_and_confusions_on_a_hand_written_pair():
    from parakeet_amd.alignment import EditAlignment, confusions, edit_align
    from parakeet_amd.utils.error_rate import encode
    ref = ["sh", "iii3", "l", "e5", "b", "ei3"]
    hyp = ["sh", "iii4", "e5", "b", "ei3", "sp"]
    r, h, _, _ = encode([ref], [hyp])
    al = edit_align(r, h)
    assert isinstance(al, EditAlignment) and al.distance == 3 and al.length == 7 and (al.ref_len, al.hyp_len) == (6, 6)
    # By hand, walking back: sp is inserted; ei3, b, e5 are hits; at (l, iii4) the ids differ and D = 2, the substitution's
    # cell D(sh iii3, sh) = 1 is one less, and the substitution comes first in the tie order; at (iii3, sh) D = 1, the
    # substitution's cell D(sh, -) = 1 is not one less, the deletion's D(sh, sh) = 0 is; then sh is a hit.
    assert _np(al.ops).tolist() == [0, 2, 1, 0, 0, 0, 3]          # hit, iii3 deleted, l -> iii4, three hits, sp inserted
    assert al.counts == (4, 1, 1, 1) and al.counts.hits == 4 and al.counts.insertions == 1
    ri, hi = al.index_pairs()
    assert ri.tolist() == [0, 1, 2, 3, 4, 5, -1] and hi.tolist() == [0, -1, 1, 2, 3, 4, 5]
    conf = confusions(al, ref, hyp)
    assert dict(conf.substitutions) == {("l", "iii4"): 1} and dict(conf.deletions) == {"iii3": 1} and dict(conf.insertions) == {"sp": 1}
    two = edit_align([r, h], [h, h])
    conf = confusions(two, [ref, hyp], [hyp, hyp])
    assert two[1].distance == 0 and two[1].counts == (6, 0, 0, 0) and dict(conf.substitutions) == {("l", "iii4"): 1}
    with pytest.raises(ValueError, match="alignment 0 is one of a 6 x 6 pair"):
        confusions([al], [ref[:2]], [hyp])


# ------------------------------------------------------------------------------------------------------------- the recipes
def _want_report(ref_tokens, hyp_tokens, k):
    """Distances, lengths and the confusion report from the restatement."""
    import collections
    from parakeet_amd.utils.error_rate import encode, format_confusions
    Conf = collections.namedtuple("Conf", "substitutions deletions insertions")
    conf = Conf(collections.Counter(), collections.Counter(), collections.Counter())
    dist, rows = [], []
    for rt, ht in zip(ref_tokens, hyp_tokens):
        r, h, _, _ = encode([rt], [ht])
        al = er.align(r, h)
        ri, hi = er.index_pairs(al["ops"])
        for op, i, j in zip(al["ops"], ri, hi):
            if op == er.SUB:
                conf.substitutions[(rt[i], ht[j])] += 1
            elif op == er.DEL:
                conf.deletions[rt[i]] += 1
            elif op == er.INS:
                conf.insertions[ht[j]] += 1
        dist.append(al["distance"])
        rows.append([al["distance"], len(rt)] + al["counts"][1:].tolist())
    return dist, rows, format_confusions(conf, k)


def test_g2p_recipe_end_to_end(tmp_path, capsys):
    import frontend_g2p_wer as ex
    from parakeet_amd.frontend import Frontend
    with open(os.path.join(HERE, "golden", "zh_frontend.json"), "rt", encoding="utf-8") as f:
        texts = [t for t in json.load(f)["phonemes"] if " " not in t and "|" not in t][:5]
    assert len(texts) == 5
    fe = Frontend()
    ids = [f"00000{k}" for k in range(1, 6)]
    hyp_tokens = [[p for p in sum(fe.get_phonemes(ex.text_cleaner(t)), []) if p not in ex.SILENCE_TOKENS] for t in texts]
    assert all(len(h) >= 4 for h in hyp_tokens)
    # the labels: the frontend's own phones with one changed, one dropped, one added (per sentence in turn) and silences in between
    labels = []
    for k, h in enumerate(hyp_tokens):
        lab = list(h)
        if k % 3 == 0:
            lab[1] = f"zz{k}"
        elif k % 3 == 1:
            del lab[2]
        else:
            lab.insert(3, "ng1")
        labels.append(lab)
    os.makedirs(tmp_path / "in")
    (tmp_path / "in" / "text").write_text("".join(f"{u} {t[:2]}#1{t[2:]}\n" for u, t in zip(ids, texts)) + "000009 没有标注\n", encoding="utf-8")
    (tmp_path / "in" / "text.ref").write_text("".join(f"{u} sil {' '.join(lab[:2])} sp1 {' '.join(lab[2:])} sp\n" for u, lab in zip(ids, labels)), encoding="utf-8")
    capsys.readouterr()
    out = ex.main(["--input-dir", str(tmp_path / "in"), "--output-dir", str(tmp_path / "out"), "--confusions", "3",
                   "--per-utterance", str(tmp_path / "per.txt")])
    text = capsys.readouterr().out
    dist, rows, report = _want_report(labels, hyp_tokens, 3)
    rate = float(sum(dist)) / sum(len(lab) for lab in labels)
    assert sum(dist) == 5 and out["rate"] == rate and out["utt_ids"] == ids and out["distances"].tolist() == [float(d) for d in dist]
    assert text.splitlines()[-1] == f"The avg WER of g2p is: {rate}"
    assert text.splitlines()[:-1] == report == out["report"] and "1\tzz0 -> " + hyp_tokens[0][1] in report
    assert (tmp_path / "out" / "text.g2p").read_text(encoding="utf-8") == "".join(f"{' '.join(h)}(baker_{u})\n" for u, h in zip(ids, hyp_tokens))
    assert (tmp_path / "out" / "text.ref.clean").read_text(encoding="utf-8") == "".join(f"{' '.join(lab)}(baker_{u})\n" for u, lab in zip(ids, labels))
    assert (tmp_path / "per.txt").read_text() == "".join(f"{u} {' '.join(str(v) for v in row)}\n" for u, row in zip(ids, rows))
    capsys.readouterr()
    plain = ex.main(["--input-dir", str(tmp_path / "in"), "--output-dir", str(tmp_path / "out2")])      # mode 0 alone
    assert plain["rate"] == rate and plain["report"] is None and capsys.readouterr().out == f"The avg WER of g2p is: {rate}\n"


def test_textnorm_recipe_end_to_end(tmp_path, capsys):
    import frontend_textnorm_cer as ex
    from parakeet_amd.frontend import TextNormalizer
    from parakeet_amd.utils.error_rate import split_chars
    raws = ["今天是2021年3月5日。", "电话10086转ABC", "气温-3°C，很冷", "他有12个苹果和3.5斤梨", "没有数字的一句话"]
    ids = [f"t{k}" for k in range(5)]
    tn = TextNormalizer()
    normed = [tn.normalize_sentence(r) for r in raws]
    labels = [normed[0], normed[1].replace("一", "幺"), normed[2] + "啊", normed[3][1:], "ok" + normed[4]]
    assert labels[1] != normed[1]
    os.makedirs(tmp_path / "in")
    (tmp_path / "in" / "text").write_text("".join(f"{u} {r}\n" for u, r in zip(ids, raws)), encoding="utf-8")
    (tmp_path / "in" / "text.ref").write_text("".join(f"{u} {lab}\n" for u, lab in zip(ids, labels)) + "t9 多余\n", encoding="utf-8")
    capsys.readouterr()
    out = ex.main(["--input-dir", str(tmp_path / "in"), "--output-dir", str(tmp_path / "out"), "--confusions", "2",
                   "--per-utterance", str(tmp_path / "per.txt")])
    text = capsys.readouterr().out
    gts, tns = [ex.del_en_add_space(lab) for lab in labels], [ex.del_en_add_space(x) for x in normed]
    ref_tokens, hyp_tokens = [split_chars(g) for g in gts], [split_chars(t) for t in tns]
    dist, rows, report = _want_report(ref_tokens, hyp_tokens, 2)
    rate = float(sum(dist)) / sum(len(r) for r in ref_tokens)
    assert sum(dist) > 0 and dist[0] == 0 and dist[4] == 0 and out["rate"] == rate and out["utt_ids"] == ids
    assert text.splitlines()[-1] == f"The avg CER of text normalization is: {rate}"
    assert text.splitlines()[:-1] == report == out["report"]
    assert (tmp_path / "out" / "text.tn").read_text(encoding="utf-8") == "".join(f"{t}({u})\n" for u, t in zip(ids, tns))
    assert (tmp_path / "out" / "text.ref.clean").read_text(encoding="utf-8") == "".join(f"{g}({u})\n" for u, g in zip(ids, gts))
    assert (tmp_path / "per.txt").read_text() == "".join(f"{u} {' '.join(str(v) for v in row)}\n" for u, row in zip(ids, rows))
