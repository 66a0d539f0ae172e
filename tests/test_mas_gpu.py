"""Monotonic alignment search and focus rate on the engine (csrc/align.hip) against the fp64 restatement
tests/mas_ref.py, through the C ABI and through ``parakeet_amd.alignment``.

The forward pass is one IEEE float64 addition per cell, so durations, path and score are compared with ``==`` (the score bit
for bit); no tolerance is involved.  The issue's shapes T in {1, 2, 63, 64, 65, 127, 128, 129, 1024} x S in {T, T + 1, 2 T + 3}
are all kept; two of them (T = 1024 with S = 1025 and 2051) exceed its S * T <= 2^20 guideline and still take well under a
second each.

Attention mode.  The bound on the read-back scores is twice the accuracy HIP documents for ``logf``.  The ROCm tree this
project builds against ships no math accuracy table (no document or header under its root states an ulp figure for ``logf``);
the figure used is the 2 ulp of the HIP programming guide's "math API" table, the one tests/fp32_bounds.py and
tests/stft_loss_ref.py already rely on, so the bound is 4 ulp of the float32 result.  Largest observed error / bound on the
MI355X: 0.52 (the SWEEP-RATIO line the test prints; recorded in DESIGN.md 4.7)."""
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
import mas_ref as mr  # noqa: E402
from ar_cases import T2_CASES  # noqa: E402
from parakeet_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

LOGF_ULP = 2                      # HIP math API table: logf, maximum ulp error (see the module docstring)
SHAPES = [(S, T) for T in (1, 2, 63, 64, 65, 127, 128, 129, 1024) for S in (T, T + 1, 2 * T + 3)]
SMALL = [i for i, (S, T) in enumerate(SHAPES) if T <= 129]
_cache = {}


def _np(t):
    return t.as_subclass(torch.Tensor).detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _scores(S, T, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.standard_normal((S, T)).astype(np.float32)
    if kind == "quantised":
        return rng.integers(0, 3, size=(S, T)).astype(np.float32)
    return np.full((S, T), -0.75, dtype=np.float32)


def _cases(kind):
    """The shapes' scores and their reference results, computed once."""
    if kind not in _cache:
        vs = [_scores(S, T, kind, 100 * i + 7) for i, (S, T) in enumerate(SHAPES)]
        _cache[kind] = (vs, [mr.mas(v) for v in vs])
    return _cache[kind]


def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _call(buf, offs, row_stride, rows, cols, mode=0, eps=1e-8, want_v=False, check=True):
    """pk_mas_run on a flat float32 host buffer -> (status code, dict of per-utterance numpy results)."""
    from parakeet_amd import _capi
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    t = ctx.to_device(np.ascontiguousarray(buf, dtype=np.float32).reshape(-1))
    rows, cols = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(cols, dtype=np.int32)
    offs = None if offs is None else np.ascontiguousarray(offs, dtype=np.int64)
    B = int(rows.size)
    r64, c64 = rows.astype(np.int64), cols.astype(np.int64)
    dur = ctx.empty((max(int(c64.sum()), 1),), dtype=torch.int32)
    path = ctx.empty((max(int(r64.sum()), 1),), dtype=torch.int32)
    score = ctx.empty((B,), dtype=torch.float64)
    status = ctx.empty((B,), dtype=torch.int32)
    v = ctx.empty((int((r64 * c64).sum()),)) if want_v else None
    rc = ctx.lib.pk_mas_run(ctx.handle, dptr(t), _ptr(offs, C.c_int64), int(row_stride), _ptr(rows, C.c_int32),
                            _ptr(cols, C.c_int32), B, int(mode), float(eps), dptr(dur), dptr(path), dptr(score), dptr(status),
                            None if v is None else dptr(v))
    if rc != 0:
        if check:
            _capi.check(rc)
        return rc, ctx.lib.pk_last_error().decode()
    d, p, sc, st = _np(dur), _np(path), _np(score), _np(status)
    co, ro, vo = np.concatenate(([0], np.cumsum(c64))), np.concatenate(([0], np.cumsum(r64))), np.concatenate(([0], np.cumsum(r64 * c64)))
    out = [dict(durations=d[co[b]:co[b + 1]], path=p[ro[b]:ro[b + 1]], score=sc[b], status=int(st[b])) for b in range(B)]
    if want_v:
        vv = _np(v)
        for b in range(B):
            out[b]["v"] = vv[vo[b]:vo[b + 1]].reshape(int(rows[b]), int(cols[b]))
    return 0, out


def _packed(vs, order, gap=3):
    """The utterances in ``order``, each at an offset of its own in one buffer whose every other entry is NaN."""
    offs, o = [], gap
    for i in order:
        offs.append(o)
        o += vs[i].size + gap
    buf = np.full(o, np.nan, dtype=np.float32)
    for i, off in zip(order, offs):
        buf[off:off + vs[i].size] = vs[i].reshape(-1)
    return buf, offs, 0, [vs[i].shape[0] for i in order], [vs[i].shape[1] for i in order]


def _same(got, want, what):
    assert got["status"] == 0, what
    assert np.array_equal(got["durations"], want["durations"]), what
    assert np.array_equal(got["path"], want["path"]), what
    assert np.float64(got["score"]).view(np.int64) == np.float64(want["score"]).view(np.int64), (what, got["score"], want["score"])
    assert got["durations"].min() >= 1 and got["durations"].sum() == len(want["path"])


@pytest.mark.parametrize("kind", ["random", "quantised", "equal"])
def test_exact_in_a_ragged_batch_in_two_orders(kind):
    vs, refs = _cases(kind)
    order = list(range(len(SHAPES)))
    for od in (order, order[::-1]):
        _, got = _call(*_packed(vs, od))
        for k, i in enumerate(od):
            _same(got[k], refs[i], (kind, SHAPES[i]))
    if kind == "equal":
        for (S, T), r in zip(SHAPES, refs):
            assert r["durations"].tolist() == [1] * (T - 1) + [S - T + 1]
    for (S, T), r in zip(SHAPES, refs):
        if S == T:
            assert r["path"].tolist() == list(range(S))          # every step forced


def test_each_utterance_alone_and_contiguous():
    vs, refs = _cases("random")
    for i, v in enumerate(vs):
        _, got = _call(v, None, 0, [v.shape[0]], [v.shape[1]])
        _same(got[0], refs[i], SHAPES[i])
    sub = SMALL[::3]
    _, got = _call(np.concatenate([vs[i].reshape(-1) for i in sub]), None, 0, [SHAPES[i][0] for i in sub], [SHAPES[i][1] for i in sub])
    for k, i in enumerate(sub):
        _same(got[k], refs[i], SHAPES[i])


@pytest.mark.parametrize("kind", ["random", "quantised"])
def test_padded_tensor_with_poisoned_padding(kind):
    from parakeet_amd.alignment import monotonic_align
    vs, refs = _cases(kind)
    Sm, Tm = max(SHAPES[i][0] for i in SMALL), max(SHAPES[i][1] for i in SMALL)
    pad = np.full((len(SMALL), Sm, Tm), np.nan, dtype=np.float32)
    for k, i in enumerate(SMALL):
        pad[k, :SHAPES[i][0], :SHAPES[i][1]] = vs[i]
    rows, cols = [SHAPES[i][0] for i in SMALL], [SHAPES[i][1] for i in SMALL]
    _, got = _call(pad, np.arange(len(SMALL)) * Sm * Tm, Tm, rows, cols)
    for k, i in enumerate(SMALL):
        _same(got[k], refs[i], SHAPES[i])
    # the same through the Python interface: a padded device tensor, a list of host arrays, one map
    d, sc, p = monotonic_align(torch.from_numpy(pad), rows, cols, return_path=True)
    d2, sc2 = monotonic_align([vs[i] for i in SMALL])
    for k, i in enumerate(SMALL):
        assert np.array_equal(d[k], refs[i]["durations"]) and np.array_equal(p[k], refs[i]["path"]) and sc[k] == refs[i]["score"]
        assert np.array_equal(d2[k], d[k]) and sc2[k] == sc[k] and d[k].dtype == np.int32
    d1, s1 = monotonic_align(vs[SMALL[5]])
    assert np.array_equal(d1, refs[SMALL[5]]["durations"]) and s1 == refs[SMALL[5]]["score"] and isinstance(s1, float)


def test_both_decision_stores():
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    w = C.c_int32()
    assert ctx.lib.pk_mas_lds_words(C.byref(w)) == 0
    lds = int(w.value)
    assert 1024 <= lds <= 40960
    shapes = [(lds // 2, 64), (lds // 2 + 1, 64), (lds // 6, 130), (lds // 6 + 1, 130), (16384, 5), (8192, 128)]
    assert [mr.decision_words(S, T) <= lds for S, T in shapes] == [True, False, True, False, False, False]
    assert all(S * T <= 2 ** 20 for S, T in shapes)
    vs = [_scores(S, T, "quantised" if k % 2 else "random", 900 + k) for k, (S, T) in enumerate(shapes)]
    refs = [mr.mas(v) for v in vs]
    _, got = _call(*_packed(vs, list(range(len(vs)))))
    for k in range(len(vs)):
        _same(got[k], refs[k], shapes[k])
    for k in (1, 4):                                             # the global store alone: the workspace starts at this utterance
        _, one = _call(vs[k], None, 0, [shapes[k][0]], [shapes[k][1]])
        _same(one[0], refs[k], shapes[k])


def test_status():
    from parakeet_amd.alignment import monotonic_align
    rng = np.random.default_rng(12)
    v = rng.standard_normal((70, 66)).astype(np.float32)
    ref = mr.mas(v)
    unreachable = v.copy()
    unreachable[np.triu_indices(70, 1, 66)] = np.nan              # t > s only
    assert mr.mas(unreachable)["status"] == 0
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = v.copy()
        bad[40, 17] = bad_value
        assert mr.mas(bad)["status"] == 1
        _, got = _call(*_packed([v, bad, unreachable], [0, 1, 2]))
        assert [g["status"] for g in got] == [0, 1, 0]
        _same(got[0], ref, "clean")
        _same(got[2], ref, "NaN where t > s")
        with pytest.raises(FloatingPointError, match=r"utterance\(s\) \[1\]"):
            monotonic_align([v, bad, unreachable])
    d, _ = monotonic_align(unreachable)
    assert np.array_equal(d, ref["durations"])


def _attention(S, T, seed):
    rng = np.random.default_rng(seed)
    a = np.exp(4.0 * rng.standard_normal((S, T)))
    a = (a / a.sum(axis=1, keepdims=True)).astype(np.float32)
    a[rng.random((S, T)) < 0.05] = 0.0                           # below eps
    a[rng.random((S, T)) < 0.05] = 3e-9
    a[rng.random((S, T)) < 0.02] = 1.0
    return a


def test_attention_mode():
    from parakeet_amd.alignment import durations_from_attention
    shapes = [(37, 9), (130, 65), (64, 64), (300, 129), (5, 1)]
    maps = [_attention(S, T, 40 + k) for k, (S, T) in enumerate(shapes)]
    worst = 0.0
    for eps in (1e-8, 1e-5):
        _, got = _call(*_packed(maps, list(range(len(maps)))), mode=1, eps=eps, want_v=True)
        for a, g in zip(maps, got):
            want = mr.attention_scores_f64(a, eps)
            bound = 2 * LOGF_ULP * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            err = np.abs(g["v"].astype(np.float64) - want)
            exact = want == 0.0
            assert np.all(g["v"][exact] == 0.0)
            worst = max(worst, float((err[~exact] / bound[~exact]).max(initial=0.0)))
            _same(g, mr.mas(g["v"]), a.shape)                     # the search ran on exactly these scores
    print(f"SWEEP-RATIO mas attention scores against fp64 log, bound {2 * LOGF_ULP} ulp: {worst:.4f}")
    assert worst <= 1.0
    # the Python interface: device tensors, the post-step, the scores handed back
    from parakeet_amd.runtime import Context
    dev = [Context.get().to_device(a) for a in maps[:4]]
    d, sc, v = durations_from_attention(dev, reduction_factor=3, merge_last=True, return_scores=True)
    for k in range(4):
        ref = mr.mas(_np(v[k]))
        assert np.array_equal(d[k], mr.post_step(ref["durations"], 3, True)) and sc[k] == ref["score"]
        assert d[k].sum() == 3 * shapes[k][0] and len(d[k]) == shapes[k][1] - 1 and d[k].dtype == np.int32
    plain, _ = durations_from_attention(maps[0])
    assert np.array_equal(plain, mr.mas(_np(v[0]))["durations"])


def test_focus_rate_and_select_map():
    from parakeet_amd.alignment import focus_rate, select_map
    from parakeet_amd.runtime import Context
    shapes = [(37, 9), (130, 65), (1, 1), (301, 200)]
    utts = [np.stack([_attention(S, T, 70 + 10 * k + g) for g in range(6)]).reshape(2, 3, S, T) for k, (S, T) in enumerate(shapes)]
    want = [np.array([[mr.focus_rate(u[l, h]) for h in range(3)] for l in range(2)]) for u in utts]
    got = focus_rate(utts)
    packed = Context.get().to_device(np.concatenate([u.reshape(-1) for u in utts]))
    views, o = [], 0
    for u in utts:                                               # views of one device tensor: addressed in place
        views.append(packed[o:o + u.size].view(u.shape))
        o += u.size
    in_place = focus_rate(views)
    Sm, Tm = max(s for s, _ in shapes), max(t for _, t in shapes)
    pad = np.full((len(utts), 2, 3, Sm, Tm), np.nan, dtype=np.float32)
    for k, u in enumerate(utts):
        pad[k, :, :, :u.shape[2], :u.shape[3]] = u
    padded = focus_rate(pad, [s for s, _ in shapes], [t for _, t in shapes])
    picks = select_map(utts)
    for k, (S, T) in enumerate(shapes):
        assert got[k].shape == (2, 3) and got[k].dtype == np.float64
        assert np.all(np.abs(got[k] - want[k]) <= S * 2.0 ** -52 * want[k]), (S, T)
        assert np.array_equal(in_place[k], got[k]) and np.array_equal(padded[k], got[k])
        top = np.sort(want[k].reshape(-1))[::-1]
        if top[0] - top[1] > 2 * S * 2.0 ** -52 * top[0]:
            assert picks[k] == tuple(int(i) for i in np.unravel_index(np.argmax(want[k]), (2, 3)))
    assert any(p != (0, 0) for p in picks)
    one = focus_rate(utts[0][1, 2])
    assert one.shape == () and one == got[0][1, 2] and select_map(utts[1]) == picks[1]


def test_envelope_raises_and_launches_nothing():
    from parakeet_amd import alignment as al
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    tiny = np.zeros(4, np.float32)
    ctx.sync()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        rc, msg = _call(tiny, None, 0, [1025], [1025], check=False)
        assert rc == -3 and "1025 tokens" in msg and "1024" in msg
        rc, msg = _call(tiny, None, 0, [16385], [2], check=False)
        assert rc == -3 and "16385 rows" in msg and "16384" in msg
        rc, msg = _call(tiny, None, 0, [4, 2], [2, 3], check=False)
        assert rc == -1 and "utterance 1" in msg and "more tokens" in msg
        rc, msg = _call(tiny, None, 0, [4, 0], [2, 0], check=False)
        assert rc == -1 and "utterance 1 is empty" in msg
        rc, msg = _call(tiny, None, 0, [2], [2], mode=1, eps=0.0, check=False)
        assert rc == -1 and "eps" in msg
        assert not any(k.startswith("mas") for k in ctx.prof_dump())
        v = np.random.default_rng(1).standard_normal((9, 4)).astype(np.float32)
        _, got = _call(v, None, 0, [9], [4])
        _same(got[0], mr.mas(v), "after the refusals")
        assert ctx.prof_dump()["mas"][0] == 1
    finally:
        ctx.prof_enable(False)
    with pytest.raises(NotImplementedError, match="1024"):
        al.monotonic_align(np.zeros((1025, 1025), np.float32))
    with pytest.raises(NotImplementedError, match="16384"):
        al.durations_from_attention(np.zeros((16385, 3), np.float32))
    with pytest.raises(ValueError, match="utterance 1 has more tokens"):
        al.monotonic_align([v, v.T.copy()])
    d, _ = al.monotonic_align(v)
    assert np.array_equal(d, mr.mas(v)["durations"])


# ------------------------------------------------------------------------------------------------------------- the teachers
def _taco():
    from parakeet_amd.tacotron2 import Tacotron2
    cfg = dict(syn.TACOTRON2_LJSPEECH, **{c[0]: c[1] for c in T2_CASES}["stop"])
    m = Tacotron2(**cfg)
    m.set_state_dict(syn.tacotron2_state(cfg, seed=21, stop_bias=-8.0))
    rng = np.random.default_rng(77)
    texts = [rng.integers(1, 37, size=T) for T in (5, 3)]
    mels = [(0.5 * rng.standard_normal((L, 80))).astype(np.float32) for L in (12, 7)]
    return m.eval(), texts, mels


def test_tacotron2_durations_batch():
    from parakeet_amd.alignment import durations_from_attention, focus_rate
    m, texts, mels = _taco()
    seeds = [9, 21]
    d, sc, fr = m.durations_batch(texts, mels, seeds=seeds, return_focus=True)
    assert m.durations_batch(texts, mels, seeds=seeds)[1].tolist() == sc.tolist()
    outs = m.teacher_forced_batch(texts, mels, seeds=seeds)
    want_d, want_sc, v = durations_from_attention([o["alignments"] for o in outs], return_scores=True)
    for b in range(2):
        assert np.array_equal(d[b], want_d[b]) and sc[b] == want_sc[b]
        assert len(d[b]) == len(texts[b]) and d[b].min() >= 1 and d[b].sum() == len(mels[b])
        assert np.array_equal(d[b], mr.mas(_np(v[b]))["durations"])
        assert fr[b] == float(focus_rate(outs[b]["alignments"])) and 0.0 < fr[b] <= 1.0
    with pytest.raises(ValueError, match="utterance 1 has more tokens"):
        m.durations_batch(texts, [mels[0], mels[1][:2]], seeds=seeds)


@pytest.mark.parametrize("r", [1, 2])
def test_transformer_tts_durations_batch(r):
    from parakeet_amd.alignment import durations_from_attention, select_map
    from parakeet_amd.transformer_tts import TransformerTTS
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, elayers=1, dlayers=2, postnet_layers=2, reduction_factor=r)
    m = TransformerTTS(idim=40, odim=80, **cfg)
    m.set_state_dict(syn.transformer_tts_state(40, 80, cfg, seed=41, stop_bias=-6.0))
    m.eval()
    rng = np.random.default_rng(11)
    texts = [syn.phoneme_ids(T, idim=40, seed=500 + T) for T in (7, 3)]
    speech = [rng.standard_normal((L, 80)).astype(np.float32) for L in (23, 9)]
    seeds = [21, 22]
    d, sc = m.durations_batch(texts, speech, seeds=seeds)
    atts = [a for _, a in m.teacher_forced_batch(texts, speech, seeds=seeds)]
    picks = select_map(atts)
    assert m.last_maps == picks
    want_d, want_sc = durations_from_attention([a[l, h] for a, (l, h) in zip(atts, picks)], reduction_factor=r, merge_last=True)
    for b in range(2):
        assert tuple(atts[b].shape[2:]) == (len(speech[b]) // r, len(texts[b]) + 1)
        assert np.array_equal(d[b], want_d[b]) and sc[b] == want_sc[b]
        assert len(d[b]) == len(texts[b]) and d[b].min() >= r and d[b].sum() == (len(speech[b]) // r) * r
    named, _ = m.durations_batch(texts, speech, seeds=seeds, map=(1, 3))
    want_named, _ = durations_from_attention([a[1, 3] for a in atts], reduction_factor=r, merge_last=True)
    assert m.last_maps == [(1, 3)] * 2 and all(np.array_equal(x, y) for x, y in zip(named, want_named))
    with pytest.raises(ValueError, match="outside the model"):
        m.durations_batch(texts, speech, seeds=seeds, map=(2, 0))
    with pytest.raises(ValueError, match="focus"):
        m.durations_batch(texts, speech, seeds=seeds, map="best")


def test_example_writes_a_durations_file_the_features_example_reads(tmp_path):
    import durations_from_teacher as ex
    from fastspeech2_features import fix_durations, read_durations
    m, texts, mels = _taco()
    names = "abcdefgh"
    with open(tmp_path / "metadata.jsonl", "wt") as f:
        for b, (t, y) in enumerate(zip(texts + [texts[0]], mels + [mels[1][:3]])):      # the third: 5 tokens, 3 frames
            np.save(tmp_path / f"u{b}.npy", y)
            rec = dict(utt_id=f"u{b}", text=[int(v) for v in t], phones=[names[int(v) % 8] + str(k) for k, v in enumerate(t)],
                       mel=f"u{b}.npy")
            if b == 1:
                rec["speaker"] = "other"
            f.write(json.dumps(rec) + "\n")
    items = ex.read_metadata(str(tmp_path / "metadata.jsonl"), speaker="spk")
    report = ex.run(m, items, str(tmp_path / "out"), seed=4, batch_size=2)
    got = read_durations(str(tmp_path / "out" / "durations.txt"))
    assert list(got) == ["u0", "u1"] and got["u0"][2] == "spk" and got["u1"][2] == "other"
    want_d, want_sc = m.durations_batch(texts, mels, seeds=[4, 5])
    for b in range(2):
        phones, durs, _ = got[f"u{b}"]
        assert phones == items[b]["phones"] and durs == want_d[b].tolist()
        assert sum(durs) == len(mels[b]) and fix_durations(durs, len(mels[b])) == durs
    lines = [json.loads(line) for line in open(tmp_path / "out" / "alignment_report.jsonl")]
    by_id = {rec["utt_id"]: rec for rec in lines}
    assert lines == report and list(by_id) == ["u0", "u1", "u2"]
    assert "skipped" in by_id["u2"] and "score_per_frame" not in by_id["u2"]
    for b in range(2):
        rec = by_id[f"u{b}"]
        assert rec["frames"] == len(mels[b]) and rec["tokens"] == len(texts[b]) and 0.0 < rec["focus_rate"] <= 1.0
        assert rec["score_per_frame"] == want_sc[b] / len(mels[b]) and rec["score_per_frame"] <= 0.0
