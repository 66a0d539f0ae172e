"""The definition of DESIGN.md 4.7 on the host: the fp64 restatement (tests/mas_ref.py) against brute force over every
monotonic path, its tie rule, the duration post-step, the durations file round trip with examples/fastspeech2_features.py and
the argument checks of ``parakeet_amd.alignment`` that run before any device is touched.  No GPU is needed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import mas_ref as mr  # noqa: E402

SHAPES = [(S, T) for S in range(1, 10) for T in range(1, S + 1)]


def _scores(S, T, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.standard_normal((S, T)).astype(np.float32)
    return rng.integers(0, 3, size=(S, T)).astype(np.float32)          # {0, 1, 2}: many ties


@pytest.mark.parametrize("kind", ["random", "quantised"])
def test_restatement_is_the_best_path_by_brute_force(kind):
    for S, T in SHAPES:
        paths = mr.all_paths(S, T)
        for seed in range(3):
            v = _scores(S, T, kind, 1000 * S + 10 * T + seed)
            got = mr.mas(v)
            each = np.array([mr.path_score(v, p) for p in paths])
            assert got["status"] == 0
            assert got["score"] == each.max(), (S, T, seed)
            assert mr.path_score(v, got["path"]) == each.max()
            assert any(np.array_equal(got["path"], p) for p in paths)
            d = got["durations"]
            assert d.dtype == np.int32 and d.shape == (T,) and d.min() >= 1 and d.sum() == S
            assert np.array_equal(d, np.bincount(got["path"], minlength=T))


def test_ties_stay():
    for S, T in SHAPES + [(40, 7), (130, 129)]:
        for value in (0.0, -1.5):
            got = mr.mas(np.full((S, T), value, dtype=np.float32))
            assert got["durations"].tolist() == [1] * (T - 1) + [S - T + 1]


def test_forced_path_and_unreachable_cells():
    v = np.random.default_rng(5).standard_normal((6, 6)).astype(np.float32)
    got = mr.mas(v)
    assert got["path"].tolist() == list(range(6)) and got["score"] == mr.path_score(v, np.arange(6))
    poisoned = v.copy()
    poisoned[np.triu_indices(6, 1)] = np.nan                            # t > s: never used
    again = mr.mas(poisoned)
    assert again["status"] == 0 and again["score"] == got["score"] and np.array_equal(again["path"], got["path"])
    poisoned[4, 2] = np.inf
    assert mr.mas(poisoned)["status"] == 1


def test_post_step_and_focus_rate():
    d = np.array([3, 1, 2, 4], dtype=np.int32)
    assert mr.post_step(d).tolist() == [3, 1, 2, 4]
    assert mr.post_step(d, reduction_factor=2).tolist() == [6, 2, 4, 8]
    assert mr.post_step(d, merge_last=True).tolist() == [3, 1, 6]
    assert mr.post_step(d, 3, True).tolist() == [9, 3, 18] and mr.post_step(d, 3, True).sum() == 3 * d.sum()
    a = np.array([[0.5, 0.25, 0.25], [0.125, 0.75, 0.125]], dtype=np.float32)
    assert mr.focus_rate(a) == 0.625
    assert mr.focus_rate(np.eye(4, dtype=np.float32)) == 1.0
    x = mr.attention_scores_f64(np.array([[0.0, 1.0, 1e-9, 0.5]], dtype=np.float32), 1e-8)
    e = float(np.float32(1e-8))
    assert x.tolist() == [[np.log(e), 0.0, np.log(e), np.log(0.5)]]


def test_durations_file_round_trip(tmp_path):
    from fastspeech2_features import fix_durations, read_durations
    from parakeet_amd.alignment import write_durations
    rng = np.random.default_rng(3)
    utts = ["LJ001-0001", "b", "utt_3"]
    speakers = ["ljspeech", "spk1", "spk1"]
    phones = [["sil", "HH", "AH0", "sp"], ["a1"], ["x", "y", "x"]]
    durs = [mr.mas(rng.standard_normal((4 + 3 * len(p), len(p))).astype(np.float32))["durations"] for p in phones]
    path = str(tmp_path / "durations.txt")
    write_durations(path, utts, speakers, phones, durs)
    back = read_durations(path)
    assert list(back) == utts
    for u, spk, ph, d in zip(utts, speakers, phones, durs):
        assert back[u] == [ph, d.tolist(), spk]
        n = 4 + 3 * len(ph)
        assert sum(back[u][1]) == n and fix_durations(back[u][1], n) == d.tolist()     # the mel length stands
    write_durations(path, utts[:1], "one", phones[:1], durs[:1])                        # one speaker name for all
    assert read_durations(path)[utts[0]][2] == "one"
    with pytest.raises(ValueError, match="phones"):
        write_durations(path, utts[:1], "one", [["a", "b"]], [np.array([1])])
    with pytest.raises(ValueError, match="white space"):
        write_durations(path, utts[:1], "one", [["a b"]], [np.array([1])])
    with pytest.raises(ValueError, match="white space"):
        write_durations(path, ["u|v"], "one", [["a"]], [np.array([1])])
    with pytest.raises(ValueError, match="utterances"):
        write_durations(path, utts, speakers[:2], phones, durs)


def test_argument_checks_need_no_device():
    from parakeet_amd import alignment as al
    ok = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="utterance 1 has more tokens .3. than rows .2."):
        al.monotonic_align([ok, np.zeros((2, 3), np.float32)])
    with pytest.raises(ValueError, match="more tokens"):
        al.durations_from_attention(np.zeros((2, 4, 5), np.float32), rows=[4, 3], cols=[4, 5])
    with pytest.raises(NotImplementedError, match="1025 tokens.*1024"):
        al.monotonic_align(np.zeros((1025, 1025), np.float32))
    with pytest.raises(NotImplementedError, match="16385 rows.*16384"):
        al.monotonic_align(np.zeros((16385, 2), np.float32))
    with pytest.raises(ValueError, match="rows and cols go together"):
        al.monotonic_align(np.zeros((2, 4, 3), np.float32), rows=[4, 4])
    with pytest.raises(ValueError, match="expected a map of shape .S, T."):
        al.monotonic_align(np.zeros((2, 4, 3), np.float32))
    with pytest.raises(ValueError, match="do not lie in"):
        al.monotonic_align(np.zeros((2, 4, 3), np.float32), rows=[4, 5], cols=[3, 3])
    with pytest.raises(ValueError, match="2 utterances, 1 row counts"):
        al.monotonic_align(np.zeros((2, 4, 3), np.float32), rows=[4], cols=[3, 3])
    with pytest.raises(ValueError, match="no utterances"):
        al.monotonic_align([])
    with pytest.raises(ValueError, match="empty"):
        al.monotonic_align([np.zeros((0, 0), np.float32)])
    with pytest.raises(ValueError, match="reduction_factor"):
        al.durations_from_attention(ok, reduction_factor=0)
    with pytest.raises(ValueError, match="eps"):
        al.durations_from_attention(ok, eps=0.0)
    with pytest.raises(ValueError, match="merge_last needs at least two columns; utterance 1"):
        al.durations_from_attention([ok, np.zeros((4, 1), np.float32)], merge_last=True)
    with pytest.raises(ValueError, match="utterance 1 has maps"):
        al.focus_rate([np.zeros((2, 4, 3), np.float32), np.zeros((3, 4, 3), np.float32)])
    assert (al.MAX_TOKENS, al.MAX_ROWS) == (1024, 16384)
    header = open(os.path.join(ROOT, "parakeet_amd", "csrc", "pk_align.h")).read()
    assert "MAS_MAX_COLS = 1024;" in header and "MAS_MAX_ROWS = 16384;" in header
