"""Feature statistics on the host: the numpy restatement of csrc/pk_stats.h (tests/stats_ref.py) against an
extended-precision two-pass value under the derived bound and against scikit-learn's StandardScaler.partial_fit, the argument
and envelope checks of ``normalizer.FeatureStats`` that run before any device is touched, merge, the state_dict round trip,
``ZScore.from_stats`` and the recipe scripts compute_statistics.py -> normalize.py through the restatement.  No GPU is needed.

scikit-learn is a comparison here, never an import of the package.  The hostile corpus (offset 1e4, spread 1e-2) is judged
against the extended-precision value under the bound, not against scikit-learn, whose own result is some 1e-12 away from it."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import stats_ref as sr  # noqa: E402

DIMS = (1, 80, 513)
KINDS = ("neg5", "pos5", "unit", "neg8", "hostile", "const_col", "const_per_utt", "outlier_first", "single_row")
_cache = {}


def _case(D, kind):
    """corpus, restatement state and the extended-precision values, computed once"""
    key = (D, kind)
    if key not in _cache:
        utts = sr.corpus(D, kind, seed=1)
        st = sr.RefState(D).update(utts)
        _cache[key] = (utts, st, sr.exact(utts, D, st.K))
    return _cache[key]


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float32)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DIMS)
def test_restatement_within_the_bound_of_the_extended_precision_value(D, kind):
    utts, st, (n, mean_x, var_x, A1, S2) = _case(D, kind)
    assert st.n == n
    mean, var, _ = sr.derive(st.n, st.K, st.S1, st.S2)
    h = sr.chain_length([len(u) for u in utts], D)
    b_mean, b_var = sr.bounds(n, h, A1, S2, mean, var)
    em = np.abs(mean.astype(np.longdouble) - mean_x).astype(np.float64)
    ev = np.abs(var.astype(np.longdouble) - var_x).astype(np.float64)
    print(f"STATS-RATIO D={D} {kind}: mean {sr.ratio(em, b_mean):.3g} var {sr.ratio(ev, b_var):.3g}")
    assert np.all(em <= b_mean) and np.all(ev <= b_var)


def test_the_bound_rejects_an_unshifted_and_a_float32_accumulation():
    """the hostile corpus: sums about K = 0 and float32 sums both miss the bound the shifted float64 order meets"""
    D = 80
    utts, st, (n, mean_x, var_x, A1, S2) = _case(D, "hostile")
    mean, var, _ = sr.derive(st.n, st.K, st.S1, st.S2)
    _, b_var = sr.bounds(n, sr.chain_length([len(u) for u in utts], D), A1, S2, mean, var)
    x = np.concatenate(utts, 0)
    x64 = x.astype(np.float64)
    var_unshifted = np.maximum((x64 * x64).sum(0) - x64.sum(0) ** 2 / n, 0) / n
    d32 = x - st.K[None]
    var_f32 = (np.maximum((d32 * d32).sum(0, dtype=np.float32) - d32.sum(0, dtype=np.float32) ** 2 / np.float32(n), 0) / np.float32(n))
    assert np.any(np.abs(var_unshifted.astype(np.longdouble) - var_x) > b_var)
    assert np.any(np.abs(var_f32.astype(np.longdouble) - var_x) > b_var)


@pytest.mark.parametrize("kind", ("neg5", "pos5", "unit", "neg8", "const_col", "const_per_utt", "outlier_first"))
@pytest.mark.parametrize("D", DIMS)
def test_restatement_against_scikit_learn(D, kind):
    pre = pytest.importorskip("sklearn.preprocessing")
    utts, st, _ = _case(D, kind)
    sk = pre.StandardScaler()
    for u in utts:
        if len(u):
            sk.partial_fit(u)
    want = np.stack([sk.mean_, sk.scale_]).astype(np.float32)
    got = sr.stats_f32(st.n, st.K, st.S1, st.S2)
    assert int(sk.n_samples_seen_) == st.n
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= _ulp32(want))
    mean, var, scale = sr.derive(st.n, st.K, st.S1, st.S2)
    from sklearn.preprocessing import _data
    sk_const = _data._is_constant_feature(sk.var_, sk.mean_, sk.n_samples_seen_)
    assert np.array_equal(scale == 1.0, sk.scale_ == 1.0) and np.array_equal(scale == 1.0, sk_const)
    if kind == "const_col":
        assert scale[0] == 1.0 and mean[0] == 3.25 and var[0] == 0.0


def test_the_package_restates_the_constant_feature_rule():
    from parakeet_amd import normalizer as nz
    _data = pytest.importorskip("sklearn.preprocessing._data")
    rng = np.random.default_rng(5)
    n = 1000
    mean = rng.standard_normal(64) * 10.0 ** rng.integers(-3, 6, 64)
    var = np.abs(rng.standard_normal(64)) * 10.0 ** rng.integers(-40, 2, 64)
    var[:4] = 0.0
    want = _data._handle_zeros_in_scale(np.sqrt(var), copy=True, constant_mask=_data._is_constant_feature(var, mean, n))
    # a state with K = 0 that has exactly this mean and variance up to rounding: S1 = n mean, S2 = n var + S1^2 / n
    s1 = n * mean
    s2 = n * var + s1 * s1 / n
    m, v, scale = nz.derive_stats(n, np.zeros(64, np.float32), s1, s2)
    mask = _data._is_constant_feature(v, m, n)
    assert np.array_equal(scale == 1.0, mask | (np.sqrt(v) == 1.0))
    assert np.array_equal(scale, _data._handle_zeros_in_scale(np.sqrt(v), copy=True, constant_mask=mask))
    assert np.array_equal(want[:4], np.ones(4))


def test_derived_values_of_the_package_equal_the_restatement():
    from parakeet_amd.normalizer import FeatureStats
    for D in DIMS:
        utts, st, _ = _case(D, "pos5")
        fs = FeatureStats(D).load_state_dict({"dim": D, "n": st.n, "shift": st.K, "s1": st.S1, "s2": st.S2})
        mean, var, scale = sr.derive(st.n, st.K, st.S1, st.S2)
        assert fs.n_samples_seen_ == st.n
        assert fs.mean_.dtype == fs.var_.dtype == fs.scale_.dtype == np.float64
        assert np.array_equal(fs.mean_, mean) and np.array_equal(fs.var_, var) and np.array_equal(fs.scale_, scale)
        assert fs.stats().dtype == np.float32 and fs.stats().shape == (2, D)
        assert np.array_equal(fs.stats(), sr.stats_f32(st.n, st.K, st.S1, st.S2))
        assert sr.state_bytes_of(fs) == st.state_bytes()


def test_argument_and_envelope_checks_touch_no_device(monkeypatch):
    from parakeet_amd import normalizer as nz
    from parakeet_amd.runtime import Context

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(Context, "get", classmethod(no_device))
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            nz.FeatureStats(bad)
    for D in (1025, 4096):
        with pytest.raises(NotImplementedError, match="1024"):
            nz.FeatureStats(D)
        with pytest.raises(NotImplementedError, match="1024"):
            nz.stats_tile_rows(D)
    with pytest.raises(ValueError, match="shift"):
        nz.FeatureStats(4, shift=np.zeros(3))
    fs = nz.FeatureStats(4)
    for bad in (np.zeros((5, 3), np.float32), np.zeros(5, np.float32), np.zeros((2, 2, 4), np.float32)):
        with pytest.raises(ValueError, match="expected"):
            fs.partial_fit(bad)
        with pytest.raises(ValueError, match="expected"):
            fs.partial_fit_batch([np.zeros((1, 4), np.float32), bad])
        with pytest.raises(ValueError, match="expected"):
            fs.utterance_moments([bad])
    with pytest.raises(TypeError, match="list"):
        fs.partial_fit_batch(np.zeros((5, 4), np.float32))
    with pytest.raises(ValueError, match="group ids"):
        fs.fit([np.zeros((1, 4), np.float32)], groups=[0, 1])

    class Huge:                                        # only the shape is looked at before the envelope check
        shape = (2 ** 31, 4)
    with pytest.raises(NotImplementedError, match="2\\^31"):
        fs.partial_fit(Huge())
    with pytest.raises(RuntimeError, match="no rows"):
        fs.mean_
    with pytest.raises(ValueError):
        fs.load_state_dict({"dim": 5, "n": 0, "shift": None, "s1": np.zeros(5), "s2": np.zeros(5)})
    with pytest.raises(ValueError):
        fs.load_state_dict({"dim": 4, "n": 3, "shift": None, "s1": np.zeros(4), "s2": np.zeros(4)})
    with pytest.raises(ValueError):
        fs.merge(nz.FeatureStats(5))
    assert fs.partial_fit_batch([]) is fs and fs.n_samples_seen_ == 0


def test_geometry_of_the_restatement():
    assert [sr.col_width(D) for D in (1, 2, 3, 32, 33, 63, 64, 65, 1024)] == [1, 2, 4, 32, 64, 64, 64, 64, 64]
    assert [sr.tile_rows(D) for D in (1, 2, 3, 63, 64, 65, 80, 513, 1024)] == [4096, 4096, 4096, 512, 512, 256, 256, 32, 32]


def test_state_dict_round_trip_and_merge_within_the_bound():
    from parakeet_amd.normalizer import FeatureStats
    for D, kind in ((80, "pos5"), (1, "hostile"), (513, "neg5")):
        utts, st, (n, mean_x, var_x, A1, S2) = _case(D, kind)
        cut = 3
        a, b = sr.RefState(D).update(utts[:cut]), sr.RefState(D).update(utts[cut:])
        assert not np.array_equal(a.K, b.K)
        fa = FeatureStats(D).load_state_dict({"dim": D, "n": a.n, "shift": a.K, "s1": a.S1, "s2": a.S2})
        fb = FeatureStats(D).load_state_dict({"dim": D, "n": b.n, "shift": b.K, "s1": b.S1, "s2": b.S2})
        sd = fa.state_dict()
        assert sr.state_bytes_of(FeatureStats(D).load_state_dict(sd)) == a.state_bytes()
        sd["s1"][:] = 0                                # a copy, not a view of the state
        assert sr.state_bytes_of(fa) == a.state_bytes()
        assert fa.merge(fb) is fa and fa.n_samples_seen_ == n and np.array_equal(fa.shift_, a.K)
        # the bound about K_a for the whole corpus, plus what the re-shift of b's sums adds
        _, _, _, A1a, S2a = sr.exact(utts, D, a.K)
        _, _, _, A1b, S2b = sr.exact(utts[cut:], D, b.K)
        h = sr.chain_length([len(u) for u in utts], D) + 1
        b_mean, b_var = sr.bounds(n, h, A1a, S2a, fa.mean_, fa.var_)
        e1, e2 = sr.merge_slack(b.n, b.K, a.K, A1b, S2b)
        b_mean = b_mean + e1 / n
        b_var = b_var + (e2 + 2 * A1a * e1 / n) / n
        assert np.all(np.abs(fa.mean_.astype(np.longdouble) - mean_x) <= b_mean)
        assert np.all(np.abs(fa.var_.astype(np.longdouble) - var_x) <= b_var)
        # merging into an empty accumulator adopts the other's state, an empty one adds nothing
        fc = FeatureStats(D).merge(fb)
        assert sr.state_bytes_of(fc) == b.state_bytes()
        assert sr.state_bytes_of(fc.merge(FeatureStats(D))) == b.state_bytes()


def test_zscore_from_stats(tmp_path):
    from parakeet_amd.normalizer import FeatureStats, ZScore
    utts, st, _ = _case(80, "neg5")
    fs = FeatureStats(80).load_state_dict({"dim": 80, "n": st.n, "shift": st.K, "s1": st.S1, "s2": st.S2})
    fs.save(tmp_path / "speech_stats.npy")
    arr = np.load(tmp_path / "speech_stats.npy", allow_pickle=False)
    assert arr.dtype == np.float32 and np.array_equal(arr, fs.stats())
    for z in (ZScore.from_stats(tmp_path / "speech_stats.npy"), ZScore.from_stats(str(tmp_path / "speech_stats.npy")),
              ZScore.from_stats(arr), fs.zscore()):
        assert np.array_equal(z.mu, arr[0]) and np.array_equal(z.sigma, arr[1])
        x = utts[-1][:50]
        y = z.forward(x)
        assert y.dtype == np.float32 and np.array_equal(y, (x - arr[0]) / arr[1])
        assert np.array_equal(z(x), y) and np.array_equal(z.inverse(y), y * arr[1] + arr[0])
    with pytest.raises(ValueError, match="\\(2, D\\)"):
        ZScore.from_stats(np.zeros((3, 80), np.float32))


def _ref_backed_stats():
    """FeatureStats whose one launching method is the restatement: the scripts run without a device."""
    from parakeet_amd.normalizer import FeatureStats

    class RefBacked(FeatureStats):
        def _update(self, xs, lens):
            n, k, s1, s2 = self._state()
            st = sr.RefState(self.dim, k)
            st.n, st.S1, st.S2 = n, s1.copy(), s2.copy()
            st.update([np.asarray(x, np.float32) for x in xs])
            self._load(st.n, st.K, st.S1, st.S2)
    return RefBacked


def test_compute_statistics_then_normalize_round_trip(tmp_path):
    import compute_statistics as cs
    import normalize as nm
    rng = np.random.default_rng(11)
    raw = tmp_path / "dump" / "train" / "raw"
    corp = {}
    with open(os.path.join(os.makedirs(raw, exist_ok=True) or raw, "metadata.jsonl"), "wt") as f:
        for i, utt in enumerate(("u2", "u0", "u1", "u3")):
            L, T = 20 + 7 * i, 3 + i
            corp[utt] = dict(speech=sr.gaussian(rng, L, 80, -5, 2), pitch=sr.gaussian(rng, T, 1, 5.2, 0.3),
                             energy=sr.gaussian(rng, T, 1, 0, 1)[:, 0])          # (T,): a 1-D file is D = 1
            rec = dict(utt_id=utt, phones=["a", "b", "a"][:T], speaker="spk%d" % (i % 2), durations=[1] * T, text_lengths=T,
                       speech_lengths=L)
            for kind, x in corp[utt].items():
                os.makedirs(raw / f"data_{kind}", exist_ok=True)
                np.save(raw / f"data_{kind}" / f"{utt}_{kind}.npy", x)
                rec[kind] = f"data_{kind}/{utt}_{kind}.npy"
            rec["feats"] = rec["speech"]
            f.write(json.dumps(rec) + "\n")
    meta = str(raw / "metadata.jsonl")
    Ref = _ref_backed_stats()
    outs = {}
    for kind in ("speech", "pitch", "energy"):
        outs[kind] = cs.main(["--metadata", meta, "--field-name", kind, "--use-relative-path", "true", "--batch-frames", "45",
                              "--verbose", "0"], stats_cls=Ref)
        assert outs[kind] == tmp_path / "dump" / "train" / f"{kind}_stats.npy"      # the reference's default name
        got = np.load(outs[kind], allow_pickle=False)
        st = sr.RefState(got.shape[1]).update([corp[u][kind] for u in ("u2", "u0", "u1", "u3")])
        assert got.dtype == np.float32 and np.array_equal(got, sr.stats_f32(st.n, st.K, st.S1, st.S2))
        # ... whatever the batching
        other = cs.main(["--metadata", meta, "--field-name", kind, "--batch-frames", "1", "--output", str(tmp_path / "o.npy"),
                         "--verbose", "0"], stats_cls=Ref)
        assert np.array_equal(np.load(other), got)
    (tmp_path / "phones.txt").write_text("a 1\nb 2\n")
    (tmp_path / "spk.txt").write_text("spk0 0\nspk1 1\n")
    recs = nm.main(["--metadata", meta, "--dumpdir", str(tmp_path / "dump" / "train" / "norm"), "--speech-stats", str(outs["speech"]),
                    "--pitch-stats", str(outs["pitch"]), "--energy-stats", str(outs["energy"]), "--phones-dict",
                    str(tmp_path / "phones.txt"), "--speaker-dict", str(tmp_path / "spk.txt"), "--verbose", "0"])
    with open(tmp_path / "dump" / "train" / "norm" / "metadata.jsonl") as f:
        back = [json.loads(line) for line in f]
    assert back == recs and [r["utt_id"] for r in back] == ["u0", "u1", "u2", "u3"]
    for r in back:
        assert "phones" not in r and "speaker" not in r and r["spk_id"] in (0, 1) and set(r["text"]) <= {1, 2}
        assert r["feats"] == r["speech"] and os.path.isabs(r["speech"])
        for kind in ("speech", "pitch", "energy"):
            s = np.load(outs[kind])
            y = np.load(r[kind], allow_pickle=False)
            x = corp[r["utt_id"]][kind]
            assert y.dtype == np.float32 and np.array_equal(y, (x - s[0]) / s[1])
    # the normalised corpus has mean 0 and scale 1 to float32 accuracy
    allsp = np.concatenate([np.load(r["speech"]) for r in back], 0).astype(np.float64)
    assert np.abs(allsp.mean(0)).max() < 1e-5 and np.abs(allsp.std(0) - 1).max() < 1e-5
    # speech only: the SpeedySpeech / TransformerTTS / vocoder form
    recs2 = nm.main(["--metadata", meta, "--dumpdir", str(tmp_path / "norm2"), "--speech-stats", str(outs["speech"]), "--verbose", "0"])
    assert all(r["pitch"].startswith("data_pitch") and os.path.isabs(r["feats"]) and r["phones"] for r in recs2)
