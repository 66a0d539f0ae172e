"""Viterbi tracking over the pitch estimator's candidates (k_pitch_cand, k_pitch_viterbi in csrc/pitch.hip) against the float64
restatement of its definition (tests/pitch_track_ref.py).

The restatement is fed the device's own d' rows, and the definition fixes every operation and its order, so candidates, lags,
f0 and score are compared bit for bit everywhere: on the test signals, on synthetic rows that hold the edge cases, with the
backpointers in LDS and in the global workspace, alone and in a batch.  What the tracker is for is checked on the "hard
signal": the frame-by-frame picker jumps an octave there, the tracker does not.  Synthetic signals only."""
import ctypes as C
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pitch_ref as pr  # noqa: E402
import pitch_track_ref as ptr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPES = [(24000, 300), (22050, 256)]
_HANDLES = {}


def _pitch(sr=24000, hop=300, tracker="frame", f0min=80, f0max=400, **kw):
    from parakeet_amd.audio import Pitch
    key = (sr, hop, tracker, f0min, f0max, tuple(sorted(kw.items())))
    if key not in _HANDLES:
        _HANDLES[key] = Pitch(sr, hop, f0min, f0max, tracker=tracker, **kw)
    return _HANDLES[key]


def _bits(a):
    a = np.asarray(a)
    if a.dtype.kind == "i":
        return a.astype(np.int64)
    return a.view(np.uint64) if a.dtype == np.float64 else a.astype(np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _want(p, rows):
    """the restatement on fp32 rows with the handle's parameters; f0 rounded once"""
    res = ptr.track(rows, p.sr, p.tau_min, p.tau_max, p.max_candidates, p.candidate_threshold, p.octave_cost, p.unvoiced_cost,
                    p.switch_cost)
    res["f0"] = res["f0"].astype(np.float32)
    return res


def _assert_equal(got, want, what):
    """got: dict of numpy arrays / a float score from the device; want: the restatement's"""
    assert np.array_equal(_bits(got["cand_lag"]), _bits(want["cand_lag"])), what + ": candidate lags"
    assert np.array_equal(_bits(got["cand_cost"]), _bits(want["cand_cost"])), what + ": candidate costs"
    assert np.array_equal(_bits(got["lag"]), _bits(want["lag"])), what + ": lags"
    assert np.array_equal(_bits(got["f0"]), _bits(want["f0"])), what + ": f0"
    assert np.float64(got["score"]).view(np.uint64) == np.float64(want["score"]).view(np.uint64), what + ": score"


def _from_cmnd(p, rows_list):
    return [dict(f0=_np(r["f0"]), lag=_np(r["lag"]), score=r["score"], cand_lag=_np(r["cand_lag"]), cand_cost=_np(r["cand_cost"]))
            for r in p.track_from_cmnd(rows_list)]


# ---------------------------------------------------------------------------------------------------- bit-exact
@pytest.mark.parametrize("seconds", [pr.DUR, 0.4])
@pytest.mark.parametrize("sr,hop", RECIPES)
def test_signals_bit_exact(sr, hop, seconds):
    p = _pitch(sr, hop, "viterbi")
    xs = [ptr.hard_signal(sr, 0, seconds), pr.make_signal(sr, 1, seconds)]
    rows = [_np(p.cmnd(x)) for x in xs]
    tracks = p.track_viterbi(xs, return_score=True)
    cands = p.candidates(xs)
    for name, r, (f0, lag, score), (cl, cc) in zip(("hard", "make"), rows, tracks, cands):
        want = _want(p, r)
        got = dict(f0=_np(f0), lag=_np(lag), score=score, cand_lag=_np(cl), cand_cost=_np(cc))
        _assert_equal(got, want, f"{name} {sr}/{hop} {seconds} s")
        assert (want["lag"] > 0).sum() >= 0.4 * want["lag"].size
        assert seconds < pr.DUR or (want["cand_lag"] > 0).sum(1).max() >= 2   # (0.4 s ends before the first weak stretch)


# ------------------------------------------------------------------------------------------------ synthetic rows
def _rows(rng, frames, tau_min, tau_max, kind):
    """(frames, tau_max + 1) fp32 d' rows.  Values are multiples of 1 / 16 between 0 and 1, so equal costs, plateaus and equal
    path costs are common; 'dense': many minima per frame (more than 8 at tau_max 40), 'sparse': few, and every fourth
    frame has none; 'none': no value under theta_c anywhere (an all-unvoiced track)."""
    if kind == "none":
        return np.float32(rng.integers(12, 17, (frames, tau_max + 1)) / 16.0)
    r = rng.integers(0, 17, (frames, tau_max + 1)) / 16.0
    if kind == "sparse":
        r = np.maximum(r, 0.75)
        for i in range(frames):
            if i % 4 != 3:
                for t in rng.choice(np.arange(tau_min, tau_max), int(rng.integers(1, 4)), replace=False):
                    r[i, t] = rng.integers(0, 5) / 16.0
        r[0, tau_min - 1], r[0, tau_min] = 1.0, 0.125                 # minima at tau_min and at tau_max - 1
        r[-1, tau_max - 2], r[-1, tau_max - 1], r[-1, tau_max] = 1.0, 0.125, 0.125
    return np.float32(r)


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("tau_max,kind", [(12, "dense"), (25, "sparse"), (40, "dense"), (40, "sparse"), (31, "none")])
def test_track_from_cmnd_on_synthetic_rows(tau_max, kind, K):
    sr = 8000
    for cu, sw in ((0.1, 0.05), (0.0, 0.0), (0.25, 0.0)):
        p = _pitch(sr, 64, "viterbi", f0min=Fraction(sr, tau_max), f0max=2000, max_candidates=K, unvoiced_cost=cu, switch_cost=sw,
                   octave_cost=0.5)
        assert (p.tau_min, p.tau_max) == (4, tau_max)
        rng = np.random.default_rng(tau_max * 10 + K)
        rows = [_rows(rng, n, p.tau_min, tau_max, kind) for n in (1, 2, 63, 64, 65, 130)]
        got = _from_cmnd(p, rows)
        t = np.arange(p.tau_min, tau_max)
        n_cand = n_min = 0
        empty = plateau = False
        for r, g in zip(rows, got):
            want = _want(p, r)
            _assert_equal(g, want, f"tau_max {tau_max} {kind} K {K} cu {cu} sw {sw}, {r.shape[0]} frames")
            minima = (r[:, t] < r[:, t - 1]) & (r[:, t] <= r[:, t + 1]) & (r[:, t] < 0.5)
            n_min = max(n_min, int(minima.sum(1).max()))
            n_cand = max(n_cand, int((want["cand_lag"] > 0).sum(1).max()))
            empty |= bool(((want["cand_lag"] > 0).sum(1) == 0).any())
            plateau |= bool((minima & (r[:, t] == r[:, t + 1])).any())
            if kind == "none":
                assert not want["lag"].any() and not g["f0"].any() and not want["cand_lag"].any()
        assert n_cand == min(K, n_min)
        if kind == "sparse":
            assert empty                                              # frames with no candidate
        if kind == "dense":
            assert plateau and n_min > (8 if tau_max == 40 else 3)    # more minima than slots


def test_candidate_edges():
    """One hand-made row: minima at tau_min and tau_max - 1, a plateau, equal costs, values at and above the threshold."""
    p = _pitch(8000, 64, "viterbi", f0min=500, f0max=2000, max_candidates=3)
    assert (p.tau_min, p.tau_max) == (4, 16)
    r = np.ones((1, 17), np.float32)
    r[0, [4, 7, 8, 10, 12, 15]] = [0.25, 0.125, 0.125, 0.25, 0.5, 0.0625]
    g = _from_cmnd(p, [r])[0]
    assert list(g["cand_lag"][0]) == [4, 7, 15]                       # 15, 7 (not 8: <=), then 4 before 10 (equal cost: the lag)
    assert list(g["cand_cost"][0]) == [0.25, 0.125, 0.0625]
    assert g["lag"][0] == 15 and g["score"] == 0.0625
    p8 = _pitch(8000, 64, "viterbi", f0min=500, f0max=2000)
    g = _from_cmnd(p8, [r])[0]
    assert list(g["cand_lag"][0]) == [4, 7, 10, 15, 0, 0, 0, 0]        # 12 is not under theta_c = 0.5
    assert np.all(np.isposinf(g["cand_cost"][0, 4:]))
    _assert_equal(g, _want(p8, r), "hand-made row")


# ------------------------------------------------------------------------------------------------ workspace path
@pytest.mark.parametrize("limit", [1, 64, 99])
def test_workspace_backpointers_equal_lds(limit):
    from parakeet_amd.audio import Pitch
    sr, hop = 22050, 256
    x = ptr.hard_signal(sr, 1)[:129 * hop]                            # 130 frames
    short = x[:99 * hop]                                              # 100 frames
    p = _pitch(sr, hop, "viterbi")
    lds = p.track_viterbi([x, short, x[:40 * hop]], return_score=True)
    q = Pitch(sr, hop, 80, 400, tracker="viterbi")
    q.set_track_lds_frames(limit)
    ws = q.track_viterbi([x, short, x[:40 * hop]], return_score=True)
    assert lds[0][0].shape == (130,) and lds[1][0].shape == (100,)
    for a, b in zip(lds, ws):
        assert np.array_equal(_bits(_np(a[0])), _bits(_np(b[0]))) and np.array_equal(_np(a[1]), _np(b[1])) and a[2] == b[2]
    want = _want(p, _np(p.cmnd(x)))
    assert np.array_equal(_np(ws[0][1]), want["lag"]) and ws[0][2] == want["score"] and (want["lag"] > 0).sum() > 60
    with pytest.raises(ValueError):
        q.set_track_lds_frames(0)
    with pytest.raises(ValueError):
        q.set_track_lds_frames(4097)


# --------------------------------------------------------------------------------------------------- consistency
def test_track_run_equals_from_cmnd_ragged_batch_and_repeat():
    sr, hop = 22050, 256
    p = _pitch(sr, hop, "viterbi")
    sig = ptr.hard_signal(sr, 2)
    rng = np.random.default_rng(5)
    lens = [1, 18687, hop - 1, hop, 64 * hop - 1, 64 * hop, 5000, 17]
    xs = [(sig[:n] if k % 3 else sig[7000:7000 + n]).copy() for k, n in enumerate(lens)]
    xs[4] = (0.3 * rng.standard_normal(lens[4])).astype(np.float32)
    assert {pr.n_frames(n, hop) for n in lens} >= {1, 2, 64, 65, 73}

    def run(ws):
        t, c = p.track_viterbi(ws, return_score=True), p.candidates(ws)
        return [(_np(a), _np(b), s, _np(cl), _np(cc)) for (a, b, s), (cl, cc) in zip(t, c)]

    def same(u, v):
        return all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(u, v))
    batch = run(xs)
    assert all(same(a, b) for a, b in zip(batch, run(xs)))            # a repeat call
    other = run(xs[::-1])[::-1]
    cm = p._run(xs, want_cmnd=True)[2]
    via = _from_cmnd(p, cm)
    for x, a, o, v in zip(xs, batch, other, via):
        assert same(a, o) and same(a, run([x])[0])
        assert same(a, (v["f0"], v["lag"], v["score"], v["cand_lag"], v["cand_cost"]))
    assert (batch[1][1] > 0).sum() > 30


# ---------------------------------------------------------------------------------------------- what it is for
@pytest.mark.parametrize("sr,hop", RECIPES)
def test_picker_jumps_an_octave_tracker_does_not(sr, hop):
    xs = [ptr.hard_signal(sr, seed) for seed in (0, 1, 2)]
    frame = _pitch(sr, hop, "frame").track(xs)
    vit = _pitch(sr, hop, "viterbi").track(xs)
    for seed, ((f0, _), (g0, _)) in enumerate(zip(frame, vit)):
        gross, _ = ptr.gross_errors(_np(f0), sr, hop)
        t_gross, t_unv = ptr.gross_errors(_np(g0), sr, hop)
        print(f"hard {sr}/{hop} seed {seed}: picker {gross.sum()} gross errors, tracker {t_gross.sum()} and {t_unv.sum()} unvoiced")
        assert gross.sum() >= 3
        assert t_gross.sum() == 0 and t_unv.sum() <= 4


def test_defaults_are_unchanged_and_get_pitch_honours_the_tracker():
    import torch
    from parakeet_amd.audio import Pitch, continuous_f0_batch
    xs = [ptr.hard_signal(24000, 0, 0.5), pr.make_signal(24000, 1, 0.3)]
    a, b = Pitch().track(xs), Pitch(tracker="frame").track(xs)
    assert all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(a, b))
    p, v = _pitch(24000, 300, "frame"), _pitch(24000, 300, "viterbi")
    assert all(torch.equal(u, w) for u, w in zip(p.get_pitch_batch(xs), v.get_pitch_batch(xs, tracker="frame")))
    raw = [f for f, _ in v.track_viterbi(xs)]
    assert all(torch.equal(f, g[0]) for f, g in zip(raw, v.track(xs)))
    assert any(not torch.equal(f, g[0]) for f, g in zip(raw, p.track(xs)))
    for got in (v.get_pitch_batch(xs), p.get_pitch_batch(xs, tracker="viterbi")):
        assert all(torch.equal(f, g) for f, g in zip(got, continuous_f0_batch(raw, use_log_f0=True)))
    assert torch.equal(v.get_pitch(xs[0]), v.get_pitch_batch(xs)[0]) and torch.equal(v._calculate_f0(xs[0]), v.get_pitch(xs[0]))
    plain = v.get_pitch_batch(xs, None, use_continuous_f0=False, use_log_f0=False)
    assert all(torch.equal(f, g) for f, g in zip(plain, raw))
    with pytest.raises(ValueError):
        p.get_pitch_batch(xs, tracker="median")
    with pytest.raises(ValueError):
        v.track_from_cmnd([np.zeros((3, 7), np.float32)])
    with pytest.raises(ValueError):
        v.track_from_cmnd([np.zeros((0, v.tau_max + 1), np.float32)])


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_refusals():
    from parakeet_amd import _capi
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    lib = ctx.lib
    p = _pitch(24000, 300, "viterbi")
    x = ctx.to_device(ptr.hard_signal(24000, 0, 0.1))
    n = x.numel()
    nf = n // 300 + 1
    cm = p.cmnd(x).contiguous()
    f0 = ctx.empty((nf,))
    lens, frames = (C.c_int32 * 2)(n, 0), (C.c_int32 * 2)(nf, 0)
    big = (C.c_int32 * 1)((1 << 22) + 1)
    good = _capi.PitchTrackCfg(8, 0.5, 1.0, 0.1, 0.05)
    run, frm = lib.pk_pitch_track_run, lib.pk_pitch_track_from_cmnd
    rest = (None, None, None, None, 0)
    for fn, data, sizes in ((run, x, lens), (frm, cm, frames)):
        assert fn(None, dptr(data), sizes, 1, C.byref(good), dptr(f0), *rest) == -1
        assert fn(p.h, None, sizes, 1, C.byref(good), dptr(f0), *rest) == -1
        assert fn(p.h, dptr(data), None, 1, C.byref(good), dptr(f0), *rest) == -1
        assert fn(p.h, dptr(data), sizes, 1, None, dptr(f0), *rest) == -1
        assert fn(p.h, dptr(data), sizes, 0, C.byref(good), dptr(f0), *rest) == -1
        assert fn(p.h, dptr(data), sizes, 2, C.byref(good), dptr(f0), *rest) == -1 and b"empty" in lib.pk_last_error()
        for bad, word in (((0, 0.5, 1.0, 0.1, 0.05), b"K"), ((9, 0.5, 1.0, 0.1, 0.05), b"K"),
                          ((8, float("nan"), 1.0, 0.1, 0.05), b"threshold"), ((8, 0.5, -1.0, 0.1, 0.05), b"lambda"),
                          ((8, 0.5, 1.0, float("nan"), 0.05), b"unvoiced_cost"), ((8, 0.5, 1.0, 0.1, -0.5), b"switch_cost"),
                          ((8, 0.5, 1.0, 0.1, float("inf")), b"switch_cost")):
            c = _capi.PitchTrackCfg(*bad)
            assert fn(p.h, dptr(data), sizes, 1, C.byref(c), dptr(f0), *rest) == -1 and word in lib.pk_last_error()
        _capi.check(fn(p.h, dptr(data), sizes, 1, C.byref(good), None, *rest))          # every output may be NULL
        _capi.check(fn(p.h, dptr(data), sizes, 1, C.byref(good), dptr(f0), *rest))
        assert np.array_equal(_bits(_np(f0)), _bits(_np(p.track_viterbi([x])[0][0])))
    assert frm(p.h, dptr(cm), big, 1, C.byref(good), dptr(f0), *rest) == -3 and b"envelope" in lib.pk_last_error()
    # host pointers give what device pointers give
    want = p.track_viterbi([x], return_score=True)[0]
    cl_want, cc_want = p.candidates([x])[0]
    xh = _np(x)
    fh, lh, sh = np.empty(nf, np.float32), np.empty(nf, np.int32), np.empty(1, np.float64)
    clh, cch = np.empty((nf, 8), np.int32), np.empty((nf, 8), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for fn, data, sizes in ((run, xh, lens), (frm, _np(cm), frames)):
        _capi.check(fn(p.h, vp(data), sizes, 1, C.byref(good), vp(fh), vp(lh), vp(sh), vp(clh), vp(cch), _capi.PK_HOST_IO))
        assert np.array_equal(_bits(fh), _bits(_np(want[0]))) and np.array_equal(lh, _np(want[1])) and sh[0] == want[2]
        assert np.array_equal(clh, _np(cl_want)) and np.array_equal(_bits(cch), _bits(_np(cc_want)))
    assert lib.pk_pitch_set_option(p.h, b"track_lds_frames", 0) == -1
    assert lib.pk_pitch_set_option(p.h, b"no_such_option", 1) == -1 and b"unknown" in lib.pk_last_error()
    assert lib.pk_pitch_set_option(None, b"track_lds_frames", 1) == -1


# ---------------------------------------------------------------------------------------------------------- example
def test_example_with_the_viterbi_tracker(tmp_path):
    """examples/fastspeech2_features.py --pitch-tracker viterbi as a fresh process, on the recordings of the estimator's example
    test and one hard signal; the pitch files are the token means of the tracker's log f0."""
    import yaml
    from parakeet_amd.audio import average_by_duration, load_wav, write_wav
    cfg = dict(fs=24000, n_fft=2048, n_shift=300, win_length=1200, window="hann", n_mels=80, fmin=80, fmax=7600, f0min=80,
               f0max=400)
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(cfg))
    (tmp_path / "wav").mkdir()
    lines = []
    for k, (utt, sr, secs) in enumerate((("a", 24000, 0.5), ("b", 48000, 0.4), ("c", 24000, 0.3), ("d", 24000, 0.5))):
        sig = ptr.hard_signal(sr, 0, secs) if utt == "d" else pr.make_signal(sr, 10 + k, secs)
        write_wav(tmp_path / "wav" / (utt + ".wav"), sig, sr, subtype="FLOAT")
        frames = int(secs * 24000) // 300 + 1
        lines.append(f"{utt}|spk|" + " ".join(f"{p} {d}" for p, d in zip(["sil", "a1", "b2", "sil"], [4, frames - 12, 5, 3])))
    (tmp_path / "durations.txt").write_text("\n".join(lines) + "\n")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "fastspeech2_features.py"), "--config", str(tmp_path / "conf.yaml"),
           "--input-dir", str(tmp_path / "wav"), "--durations", str(tmp_path / "durations.txt"), "--output-dir",
           str(tmp_path / "dump"), "--pitch-tracker", "viterbi"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [json.loads(s) for s in (tmp_path / "dump" / "metadata.jsonl").read_text().splitlines()]
    assert [r["utt_id"] for r in recs] == ["a", "b", "c", "d"]
    outs = {r["utt_id"]: (np.load(tmp_path / "dump" / r["pitch"]), r["durations"]) for r in recs}
    v = _pitch(24000, 300, "viterbi")
    for utt, (got, d) in outs.items():
        wav, _ = load_wav(str(tmp_path / "wav" / (utt + ".wav")), sr=24000)
        f0 = v.get_pitch_batch([wav])[0]
        want = _np(average_by_duration(f0, np.asarray(d, np.int64))).reshape(-1, 1)
        assert got.dtype == np.float32 and got.shape == (4, 1) and np.array_equal(_bits(got), _bits(want))
