"""The pitch estimator's definition and its host side, without a device: the fp64 restatement (tests/pitch_ref.py) on a signal
whose f0 is known and on exactly periodic input, the guards that keep the device tests from being vacuous, the steps after
the estimator against goldens made by the reference's own source (tools/make_golden_pitch.py), ``pitch_lags`` and the
envelope."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pitch_ref as pr  # noqa: E402

RECIPES = [(24000, 300), (22050, 256)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pitch_post.npz")
_TRACKS = {}


def tracked(sr, hop, seed, seconds=pr.DUR):
    """(signal, reference result) of the test signal, computed once per process"""
    key = (sr, hop, seed, seconds)
    if key not in _TRACKS:
        x = pr.make_signal(sr, seed, seconds)
        _TRACKS[key] = (x, pr.track(x, sr, hop, 80, 400))
    return _TRACKS[key]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("sr,hop", RECIPES)
def test_reference_follows_the_true_contour(sr, hop, seed):
    x, res = tracked(sr, hop, seed)
    kind, tc, seg = pr.frame_kinds(sr, hop, x.size)
    voiced = res["lag"] > 0
    in_v = kind == "v"
    err = np.abs(res["f0"][voiced & in_v] / pr.f0_true(tc[voiced & in_v]) - 1.0)
    share = (voiced & in_v).sum() / in_v.sum()
    per_silent = [int((voiced & (seg == s)).sum()) for s in pr.SILENT]
    print(f"{sr}/{hop} seed {seed}: {voiced.size} frames, {in_v.sum()} in voiced segments of which {share:.1%} voiced; "
          f"f0 error max {err.max():.4%} median {np.median(err):.4%}; voiced in noise {(voiced & (kind == 'n')).sum()}, "
          f"per silent segment {per_silent}")
    assert err.max() <= 0.01
    assert share >= 0.85
    assert not (voiced & (kind == "n")).any()
    assert max(per_silent) <= 1


@pytest.mark.parametrize("P", [60, 61, 100, 173, 299])
def test_exactly_periodic_input(P):
    sr, hop = 24000, 300
    tau_min, tau_max = pr.lags(sr, 80, 400)
    L = 3 * tau_max
    x = np.tile(np.random.default_rng(P).standard_normal(P).astype(np.float32), 4000 // P + 1)[:4000]
    res = pr.track(x, sr, hop, 80, 400)
    i = np.arange(pr.n_frames(x.size, hop))
    interior = (i * hop - L // 2 >= 0) & (i * hop - L // 2 + L <= x.size)
    assert interior.sum() >= 5
    assert np.all(res["lag"][interior] == P)
    assert np.all(res["cmnd"][interior, P] == 0.0)
    f0 = res["f0"][interior]
    assert np.all((sr / (P + 0.5) < f0) & (f0 < sr / (P - 0.5)))


@pytest.mark.parametrize("seconds", [pr.DUR, 0.4])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("sr,hop", RECIPES)
def test_gpu_f0_test_is_not_vacuous(sr, hop, seed, seconds):
    """On every signal the device f0 test uses: at most 5 % of the frames undecided at the crude eps_d, at least 40 % voiced
    and decided.  The eps_d derived from the kernel's order is no larger than the crude one."""
    _, tau_max = pr.lags(sr, 80, 400)
    crude = pr.eps_crude(2 * tau_max, tau_max)
    assert pr.eps_d(2 * tau_max, tau_max) <= crude
    _, res = tracked(sr, hop, seed, seconds)
    ok = pr.decided(res, crude)
    n = ok.size
    print(f"{sr}/{hop} seed {seed} {seconds} s: {n} frames, {n - ok.sum()} undecided, {(ok & (res['lag'] > 0)).sum()} voiced and "
          f"decided, largest kappa {res['kappa'][ok].max():.1f}")
    assert (n - ok.sum()) <= 0.05 * n
    assert (ok & (res["lag"] > 0)).sum() >= 0.40 * n


def test_steps_after_the_estimator_equal_the_reference():
    g = np.load(GOLDEN)
    names = [str(n) for n in g["names"]]
    assert len(names) >= 10
    kinds = set()
    for n in names:
        f0, d = g[n + "_f0"], g[n + "_d"]
        cont = pr.continuous_f0(f0)
        assert cont.shape == g[n + "_cont"].shape and np.abs(cont - g[n + "_cont"]).max() <= 1e-12
        assert np.abs(pr.log_f0(cont) - g[n + "_log"]).max() <= 1e-12
        assert np.abs(pr.log_f0(f0) - g[n + "_rawlog"]).max() <= 1e-12
        assert pr.average(f0, d).shape == g[n + "_avg"].shape == (d.size, 1)
        assert np.abs(pr.average(f0, d) - g[n + "_avg"]).max() <= 1e-12
        assert np.abs(pr.average(pr.log_f0(cont), d) - g[n + "_pitch"]).max() <= 1e-12
        nz = np.nonzero(f0)[0]
        kinds.add("unvoiced" if nz.size == 0 else "voiced" if nz.size == f0.size else "one" if nz.size == 1 else "gaps")
        if nz.size and nz[0] > 0:
            kinds.add("lead")
        if nz.size and nz[-1] < f0.size - 1:
            kinds.add("trail")
        if (d == 0).any():
            kinds.add("zero_duration")
    assert kinds == {"unvoiced", "voiced", "one", "gaps", "lead", "trail", "zero_duration"}
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_pitch_lags():
    from parakeet_amd.audio import pitch_lags
    assert pitch_lags(24000, 80, 400) == (60, 300)
    assert pitch_lags(22050, 80, 400) == (55, 276)
    assert pitch_lags(24000, 80, 7600) == (3, 300)           # the reference's default f0max
    assert pitch_lags(48000, 50, 400) == (120, 960)
    assert pitch_lags(16000, 80, 16000) == (2, 200)          # never below 2
    assert pitch_lags(22050, 80, 400) == pr.lags(22050, 80, 400)
    for bad in ((24000, 400, 80), (24000, 80, 80), (24000, 0, 400), (24000, 80, -1), (0, 80, 400), (-24000, 80, 400)):
        with pytest.raises(ValueError):
            pitch_lags(*bad)
    with pytest.raises(ValueError):
        pitch_lags(300, 100, 110)                            # lags 2 ... 3: tau_min > tau_max - 2
    with pytest.raises(ValueError):
        pitch_lags(400, 100, 110)                            # lags 3 ... 4


def test_refusals_need_no_device():
    """ValueError and NotImplementedError are raised before the engine is touched."""
    from parakeet_amd import audio
    assert (audio.PITCH_MAX_TAU, audio.PITCH_MAX_HOP) == (960, 16384)
    with pytest.raises(ValueError):
        audio.Pitch(24000, 300, 400, 80)
    with pytest.raises(ValueError):
        audio.Pitch(24000, 300, 80, 400, threshold=0.0)
    with pytest.raises(ValueError):
        audio.Pitch(24000, 0, 80, 400)
    for kw in (dict(sr=48000, f0min=49), dict(sr=96000, f0min=80), dict(win_length=601), dict(win_length=0),
               dict(hop_length=16385)):
        args = dict(sr=24000, hop_length=300, f0min=80, f0max=400)
        args.update(kw)
        with pytest.raises(NotImplementedError):
            audio.Pitch(**args)
    audio._check_pitch_envelope(300, 960, 1920)              # the corner of the envelope the issue asks for is inside


def test_envelope_constants_mirror_the_header():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from parakeet_amd import audio
    text = open(os.path.join(root, "parakeet_amd", "csrc", "pk_pitch.h")).read()
    val = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))   # noqa: E731
    assert (val("PT_MAX_TAU"), val("PT_MAX_HOP")) == (audio.PITCH_MAX_TAU, audio.PITCH_MAX_HOP)
    assert val("PT_R") % 2 == 1
