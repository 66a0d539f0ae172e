"""Feature statistics on the engine (csrc/stats.hip) against the numpy restatement of csrc/pk_stats.h
(tests/stats_ref.py), through ``normalizer.FeatureStats`` and the C ABI.

Every sum is a chain of single IEEE float64 additions in a stated order, so states are compared as BYTES: against the
restatement, across one batch / one by one / uneven splits, alone against inside a batch, host against device input.  Only
``mean_`` and ``var_`` against the extended-precision value use a bound, the one derived in stats_ref.py; the largest
error / bound the MI355X gave is the STATS-RATIO line each case prints (recorded in DESIGN.md 4.5g).  scikit-learn, where it
can be imported, is a comparison of the float32 (2, D) file to one float32 ulp; the hostile corpus (1e4, 1e-2) is judged
against the extended-precision value instead (scikit-learn itself is some 1e-12 away from it there).

Shapes: D in {1, 2, 3, 63, 64, 65, 80, 513, 1024}; with R = pk_stats_tile_rows(D) the lengths come from
{0, 1, 2, R - 1, R, R + 1, 2 R + 1} plus one utterance of 40 R + 3 rows."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import stats_ref as sr  # noqa: E402
from parakeet_amd import _capi  # noqa: E402
from parakeet_amd import normalizer as nz  # noqa: E402
from parakeet_amd.runtime import Context  # noqa: E402

pytestmark = pytest.mark.gpu

DIMS = (1, 2, 3, 63, 64, 65, 80, 513, 1024)
KINDS = ("neg5", "pos5", "hostile", "const_col", "const_per_utt", "outlier_first", "single_row")
_cache = {}


def _case(D, kind):
    """corpus, restatement state, extended-precision values: computed once, never modified"""
    key = (D, kind)
    if key not in _cache:
        utts = sr.corpus(D, kind, seed=2)
        st = sr.RefState(D).update(utts)
        _cache[key] = (utts, st, sr.exact(utts, D, st.K))
    return _cache[key]


def _np(t):
    return t.as_subclass(torch.Tensor).detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


@pytest.mark.parametrize("D", DIMS)
def test_tile_rows_is_the_restatement_s(D):
    assert nz.stats_tile_rows(D) == sr.tile_rows(D)
    short, long_ = sr.gpu_lengths(D)
    R = sr.tile_rows(D)
    assert short == [0, 1, 2, R - 1, R, R + 1, 2 * R + 1] and long_ // R == 40


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", DIMS)
def test_state_is_the_restatement_s_in_any_split(D, kind):
    utts, st, (n, mean_x, var_x, A1, S2) = _case(D, kind)
    want = st.state_bytes()
    one = nz.FeatureStats(D).fit(utts)
    assert sr.state_bytes_of(one) == want
    each = nz.FeatureStats(D)
    for u in utts:
        each.partial_fit(u)
    assert sr.state_bytes_of(each) == want
    for cuts in ((1,), (3, 4, 7)):                     # two uneven splits (the second has an empty call's worth in it)
        fs = nz.FeatureStats(D)
        for part in np.split(np.arange(len(utts)), [c for c in cuts if c < len(utts)]):
            fs.partial_fit_batch([utts[i] for i in part])
        assert sr.state_bytes_of(fs) == want
    assert one.n_samples_seen_ == n
    mean, var = one.mean_, one.var_
    h = sr.chain_length([len(u) for u in utts], D)
    b_mean, b_var = sr.bounds(n, h, A1, S2, mean, var)
    em = np.abs(mean.astype(np.longdouble) - mean_x).astype(np.float64)
    ev = np.abs(var.astype(np.longdouble) - var_x).astype(np.float64)
    print(f"STATS-RATIO D={D} {kind}: mean {sr.ratio(em, b_mean):.3g} var {sr.ratio(ev, b_var):.3g}")
    assert np.all(em <= b_mean) and np.all(ev <= b_var)
    assert np.array_equal(one.stats(), sr.stats_f32(st.n, st.K, st.S1, st.S2))
    if kind == "const_col":
        assert one.scale_[0] == 1.0 and one.var_[0] == 0.0 and one.mean_[0] == 3.25
    if kind == "const_per_utt" and len(utts) > 1:
        assert one.scale_[0] != 1.0 and one.var_[0] > 0
    if kind == "outlier_first":
        assert np.all(one.shift_ == 0.0)               # the shift is the silent token, the statistics still meet the bound


@pytest.mark.parametrize("kind", ("neg5", "pos5", "const_col", "const_per_utt", "outlier_first"))
@pytest.mark.parametrize("D", DIMS)
def test_stats_file_against_scikit_learn(D, kind):
    pre = pytest.importorskip("sklearn.preprocessing")
    utts, st, _ = _case(D, kind)
    sk = pre.StandardScaler()
    for u in utts:
        if len(u):
            sk.partial_fit(u)
    want = np.stack([sk.mean_, sk.scale_]).astype(np.float32)
    got = nz.FeatureStats(D).fit(utts).stats()
    assert got.dtype == np.float32 and got.shape == (2, D)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)))
    assert np.array_equal(got[1] == 1.0, want[1] == 1.0)


@pytest.mark.parametrize("D", (1, 80))
def test_batches_of_one_to_nine_utterances(D):
    R = sr.tile_rows(D)
    lens = [R + 1, 0, 2, R - 1, 1, 2 * R + 1, R, 0, 5]
    utts = sr.corpus(D, "pos5", seed=9, lens=lens)
    want = sr.RefState(D).update(utts).state_bytes()
    for k in range(1, 10):
        fs = nz.FeatureStats(D)
        for i in range(0, 9, k):
            fs.partial_fit_batch(utts[i:i + k])
        assert sr.state_bytes_of(fs) == want, k


@pytest.mark.parametrize("D", (1, 17, 80))
def test_more_utterances_than_the_fold_stages_at_a_time(D):
    """k_stats_fold stages 256 utterances' sums at a time: 256, 257 and 600 utterances in one call, a few of them empty"""
    rng = np.random.default_rng(D)
    lens = [int(v) for v in rng.integers(0, 6, 600)]
    utts = sr.corpus(D, "hostile", seed=4, lens=lens)
    for B in (256, 257, 600):
        want = sr.RefState(D).update(utts[:B]).state_bytes()
        assert sr.state_bytes_of(nz.FeatureStats(D).fit(utts[:B])) == want
        assert sr.state_bytes_of(nz.FeatureStats(D).partial_fit_batch(utts[:100]).partial_fit_batch(utts[100:B])) == want


@pytest.mark.parametrize("D", DIMS)
def test_empty_utterances_and_the_shift(D):
    x = sr.gaussian(np.random.default_rng(D), 5, D, 5.2, 0.3)
    empty = np.zeros((0, D), np.float32)
    fs = nz.FeatureStats(D)
    fs.partial_fit_batch([empty, empty, empty])        # an all-empty batch: nothing seen, the shift stays open
    assert fs.n_samples_seen_ == 0 and fs.shift_ is None
    assert sr.state_bytes_of(fs) == sr.RefState(D).state_bytes()
    fs.partial_fit_batch([empty, x[2:], x[:2]])        # the first utterance is empty: the shift comes from the second
    assert np.array_equal(fs.shift_, x[2])
    assert sr.state_bytes_of(fs) == sr.RefState(D).update([x[2:], x[:2]]).state_bytes()
    given = nz.FeatureStats(D, shift=x[4]).fit([empty, x])
    assert np.array_equal(given.shift_, x[4])
    assert sr.state_bytes_of(given) == sr.RefState(D, shift=x[4]).update([x]).state_bytes()
    assert sr.state_bytes_of(given.reset()) == sr.RefState(D, shift=x[4]).state_bytes()


@pytest.mark.parametrize("D", DIMS)
def test_utterance_moments_alone_and_in_a_batch(D):
    utts, st, _ = _case(D, "pos5")
    fs = nz.FeatureStats(D, shift=st.K)
    before = sr.state_bytes_of(fs)
    n, mean, m2 = fs.utterance_moments(utts)
    assert sr.state_bytes_of(fs) == before and fs.n_samples_seen_ == 0
    assert n.tolist() == [len(u) for u in utts] and mean.shape == m2.shape == (len(utts), D)
    for b in (0, len(utts) // 2, len(utts) - 1):
        n1, mean1, m21 = fs.utterance_moments([utts[b]])
        assert n1[0] == n[b] and mean1[0].tobytes() == mean[b].tobytes() and m21[0].tobytes() == m2[b].tobytes()
    n2, mean2, m22 = fs.utterance_moments(utts[::-1])
    assert mean2[::-1].tobytes() == mean.tobytes() and m22[::-1].tobytes() == m2.tobytes()
    for b, u in enumerate(utts):                       # ... and they are the restatement's sums
        u1, u2 = sr.utterance_sums(u, st.K)
        nf = max(len(u), 1)
        assert np.array_equal(mean[b], st.K.astype(np.float64) + u1 / nf)
        assert np.array_equal(m2[b], np.maximum(u2 - u1 * u1 / nf, 0.0))


@pytest.mark.parametrize("D", (1, 3, 80, 1024))
def test_device_and_host_input_give_equal_bytes(D):
    utts, st, _ = _case(D, "neg5")
    ctx = Context.get()
    dev = [ctx.to_device(u) for u in utts]
    a, b = nz.FeatureStats(D).fit(utts), nz.FeatureStats(D).fit(dev)
    assert sr.state_bytes_of(a) == sr.state_bytes_of(b) == st.state_bytes()
    mixed = nz.FeatureStats(D).fit([d if i % 2 else u for i, (u, d) in enumerate(zip(utts, dev))])
    assert sr.state_bytes_of(mixed) == st.state_bytes()
    if D == 1:                                         # (L,) is (L, 1)
        flat = nz.FeatureStats(1).fit([d.reshape(-1) for d in dev])
        assert sr.state_bytes_of(flat) == st.state_bytes()
    ma, mb = a.utterance_moments(utts), b.utterance_moments(dev)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ma, mb))


def test_zscore_forward_on_the_device_is_a_true_subtract_and_divide():
    utts, st, _ = _case(80, "pos5")
    z = nz.FeatureStats(80).fit(utts).zscore()
    x = np.concatenate(utts, 0)[:4000]
    want = (x - z.mu) / z.sigma                        # numpy float32: what StandardScaler.transform does to float32 input
    assert want.dtype == np.float32
    got = z.forward(Context.get().to_device(x))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32
    assert np.array_equal(_np(got).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(z.forward(x).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("D", (1, 80))
def test_groups_equal_fitting_each_group_alone(D):
    utts, st, _ = _case(D, "neg5")
    ids = ["a", "b", "a", "c", "b", "a", "c", "a"][:len(utts)]
    root = nz.FeatureStats(D)
    out = root.fit(utts, groups=ids)
    assert list(out) == ["a", "b", "c"] and root.n_samples_seen_ == 0
    for g, fs in out.items():
        mine = [u for u, i in zip(utts, ids) if i == g]
        assert sr.state_bytes_of(fs) == sr.state_bytes_of(nz.FeatureStats(D).fit(mine)) == sr.RefState(D).update(mine).state_bytes()
    # merged, the groups give the corpus' statistics within rounding
    merged = nz.FeatureStats(D)
    for fs in out.values():
        merged.merge(fs)
    assert merged.n_samples_seen_ == st.n
    whole = nz.FeatureStats(D).fit(utts)
    assert np.allclose(merged.mean_, whole.mean_, rtol=1e-12, atol=0) and np.allclose(merged.var_, whole.var_, rtol=1e-11, atol=0)


def test_state_dict_moves_a_pass_between_accumulators():
    utts, st, _ = _case(65, "pos5")
    a = nz.FeatureStats(65).partial_fit_batch(utts[:3])
    b = nz.FeatureStats(65).load_state_dict(a.state_dict())
    b.partial_fit_batch(utts[3:])                      # resumed on another accumulator: the same bytes as one pass
    assert sr.state_bytes_of(b) == st.state_bytes()
    assert sr.state_bytes_of(a) == sr.RefState(65).update(utts[:3]).state_bytes()


def test_c_abi_refuses_before_any_launch():
    ctx = Context.get()
    lib = ctx.lib
    h = C.c_void_p()
    with pytest.raises(NotImplementedError, match="1024"):
        _capi.check(lib.pk_stats_create(ctx.handle, 1025, C.byref(h)))
    with pytest.raises(NotImplementedError, match="1024"):
        _capi.check(lib.pk_stats_tile_rows(0, C.byref(C.c_int32())))
    _capi.check(lib.pk_stats_create(ctx.handle, 4, C.byref(h)))
    try:
        x = ctx.to_device(np.ones((3, 4), np.float32))
        ptr = C.c_void_p(x.data_ptr())

        def lens(*v):
            return (C.c_int64 * len(v))(*v)
        with pytest.raises(NotImplementedError, match="2\\^31"):
            _capi.check(lib.pk_stats_update(h, ptr, lens(1, 2 ** 31), 2, None, 0))
        with pytest.raises(ValueError, match="negative"):
            _capi.check(lib.pk_stats_update(h, ptr, lens(1, -1), 2, None, 0))
        with pytest.raises(ValueError, match="positive"):
            _capi.check(lib.pk_stats_update(h, ptr, lens(1), 0, None, 0))
        with pytest.raises(ValueError, match="NULL"):
            _capi.check(lib.pk_stats_update(h, None, lens(3), 1, None, 0))
        with pytest.raises(RuntimeError, match="shift"):
            out = torch.empty(8, dtype=torch.float64, device=x.device)
            _capi.check(lib.pk_stats_update(h, ptr, lens(3), 1, C.c_void_p(out.data_ptr()), _capi.PK_STATS_MOMENTS_ONLY))
        n = C.c_int64(-1)
        _capi.check(lib.pk_stats_get(h, C.byref(n), None, None, None, None))
        assert n.value == 0                            # none of the refused calls left anything behind
        _capi.check(lib.pk_stats_update(h, ptr, lens(3), 1, None, 0))
        _capi.check(lib.pk_stats_get(h, C.byref(n), None, None, None, None))
        assert n.value == 3
    finally:
        lib.pk_stats_destroy(h)


def _load_example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_features_example_writes_the_stats_of_the_files_it_wrote(tmp_path):
    import yaml
    import pitch_ref as pr
    from parakeet_amd.audio import write_wav
    cfg = dict(fs=24000, n_fft=2048, n_shift=300, win_length=1200, window="hann", n_mels=80, fmin=80, fmax=7600, f0min=80,
               f0max=400)
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(cfg))
    (tmp_path / "wav").mkdir()
    lines = []
    for k, (utt, secs) in enumerate((("a", 0.5), ("b", 0.4), ("c", 0.3))):
        write_wav(tmp_path / "wav" / (utt + ".wav"), pr.make_signal(24000, 10 + k, secs), 24000, subtype="FLOAT")
        frames = int(secs * 24000) // 300 + 1
        lines.append(f"{utt}|spk|" + " ".join(f"{p} {d}" for p, d in zip(["sil", "a1", "b2", "sil"], [4, frames - 12, 5, 3])))
    (tmp_path / "durations.txt").write_text("\n".join(lines) + "\n")
    mod = _load_example("fastspeech2_features")
    recs = mod.extract(mod.parse_args(["--config", str(tmp_path / "conf.yaml"), "--input-dir", str(tmp_path / "wav"),
                                       "--durations", str(tmp_path / "durations.txt"), "--output-dir", str(tmp_path / "dump"),
                                       "--write-stats", str(tmp_path / "stats")]))
    assert len(recs) == 3
    for kind, D in (("speech", 80), ("pitch", 1), ("energy", 1)):
        got = np.load(tmp_path / "stats" / f"{kind}_stats.npy", allow_pickle=False)
        files = [np.load(tmp_path / "dump" / r[kind], allow_pickle=False) for r in recs]
        assert got.dtype == np.float32 and got.shape == (2, D)
        assert np.array_equal(got, nz.FeatureStats(D).fit(files).stats())
        st = sr.RefState(D).update(files)
        assert np.array_equal(got, sr.stats_f32(st.n, st.K, st.S1, st.S2))
