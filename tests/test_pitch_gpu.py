"""The pitch estimator (csrc/pitch.hip) against the fp64 restatement of its definition (tests/pitch_ref.py).

d' is compared on every frame and every lag under the relative bound ``eps_d`` derived from the kernel's accumulation order
(pitch_ref.eps_d); lag and f0 on the frames the reference *decided* (every comparison its picker made has a relative margin
above 4 eps_d): there the lag must be equal and f0 within the tolerance propagated through the parabola.  Where the
arithmetic is exact (periodic input, power-of-two scaling, the same utterance in another batch) the comparison is bit for
bit.  A test asserts ratio <= 1 and prints it.

First hardware run (MI355X), largest ratio per test: see DESIGN.md 4.5e.
"""
import ctypes as C
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_bounds as fb  # noqa: E402
import pitch_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pitch_post.npz")
RECIPES = [(24000, 300), (22050, 256)]
_HANDLES, _REFS = {}, {}


def _pitch(sr=24000, hop=300):
    from parakeet_amd.audio import Pitch
    if (sr, hop) not in _HANDLES:
        _HANDLES[(sr, hop)] = Pitch(sr, hop, 80, 400)
    return _HANDLES[(sr, hop)]


def _ref(sr, hop, seed, seconds=pr.DUR):
    key = (sr, hop, seed, seconds)
    if key not in _REFS:
        x = pr.make_signal(sr, seed, seconds)
        _REFS[key] = (x, pr.track(x, sr, hop, 80, 400))
    return _REFS[key]


def _bits(a):
    a = np.asarray(a)
    return a if a.dtype.kind == "i" else (a.astype(np.float32) + np.float32(0.0)).view(np.uint32)


def _run(p, wavs):
    """-> per utterance (f0, lag, d') as numpy, one engine call"""
    f0, lag, cm = p._run(list(wavs), want_lag=True, want_cmnd=True)
    return [(a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()) for a, b, c in zip(f0, lag, cm)]


def _same(a, b):
    return all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


# -------------------------------------------------------------------------------------------------------------- d'
@pytest.mark.parametrize("sr,hop", RECIPES)
def test_cmnd_every_frame_every_lag(sr, hop):
    p = _pitch(sr, hop)
    F, W, tau_max = p.tile_frames, p.win_length, p.tau_max
    L = W + tau_max
    assert F >= 1 and W == 2 * tau_max
    lens = [1, 2, hop - 1, hop, hop + 1, L - 1, L, L + 1]
    for frames in (F - 1, F, F + 1, 3 * F + 1):
        if frames >= 1:
            lens += [max(1, (frames - 1) * hop), frames * hop - 1]
    lens = list(dict.fromkeys(lens))
    assert {F, F + 1, 3 * F + 1} <= {pr.n_frames(n, hop) for n in lens}
    rng = np.random.default_rng(sr + hop)
    sig = pr.make_signal(sr, 3)[int(0.1 * sr):]                    # from the middle of a voiced segment on
    content = [lambda n: sig[:n], lambda n: rng.standard_normal(n).astype(np.float32), lambda n: np.zeros(n, np.float32),
               lambda n: np.full(n, 0.25, np.float32)]
    xs = [content[k % 4](n).copy() for k, n in enumerate(lens)]
    for n in (L + 1, lens[-1]):                                       # the longest and L + 1 with every content
        xs += [c(n).copy() for c in content]
    got = _run(p, xs)
    eps = pr.eps_d(W, tau_max)
    worst = 0.0
    for x, (f0, lag, cm) in zip(xs, got):
        want = pr.cmnd(x, hop, tau_max, W)
        assert cm.shape == want.shape == (x.size // hop + 1, tau_max + 1) and f0.shape == lag.shape == (want.shape[0],)
        worst = max(worst, fb.ratio(cm, want, eps * np.abs(want)))
    print(f"pitch {sr}/{hop}: F {F}, {len(xs)} utterances of {min(lens)} ... {max(lens)} samples, d' ratio {worst:.4f} "
          f"(eps_d {eps:.3g})")
    assert worst <= 1.0
    # the constant: d (and so c) is 0 where the window holds no padding, d' = 1 there; elsewhere the padding enters
    x = np.full(lens[-1], 0.25, np.float32)
    cm = got[len(got) - 1][2]
    assert np.array_equal(xs[-1], x)
    i = np.arange(cm.shape[0])
    inside = (i * hop - L // 2 >= 0) & (i * hop - L // 2 + L <= x.size)
    assert inside.any() and np.all(cm[inside] == 1.0) and np.any(cm[~inside] != 1.0)


@pytest.mark.parametrize("P", [60, 61, 100, 173, 299])
def test_exactly_periodic_input(P):
    sr, hop = 24000, 300
    p = _pitch(sr, hop)
    L = p.win_length + p.tau_max
    x = np.tile(np.random.default_rng(P).standard_normal(P).astype(np.float32), 4000 // P + 1)[:4000]
    f0, lag, cm = _run(p, [x])[0]
    i = np.arange(f0.size)
    interior = (i * hop - L // 2 >= 0) & (i * hop - L // 2 + L <= x.size)
    assert interior.sum() >= 5
    assert np.all(lag[interior] == P)
    assert np.all(cm[interior, P].view(np.uint32) == 0)              # +0.0, bit for bit
    assert np.all((sr / (P + 0.5) < f0[interior]) & (f0[interior] < sr / (P - 0.5)))


def test_power_of_two_scaling_changes_no_bit():
    p = _pitch()
    x = pr.make_signal(24000, 0)
    a, b, c = _run(p, [x, x * np.float32(2.0 ** 10), x * np.float32(2.0 ** -10)])
    assert (a[1] > 0).sum() > 40
    assert _same(a, b) and _same(a, c)


@pytest.mark.parametrize("sr,hop", RECIPES)
def test_ragged_batch_is_bit_equal_to_each_utterance_alone(sr, hop):
    """Six utterances of 1 ... 3 F + 1 frames in shuffled order, each between guard utterances of 1e30 in the packed buffer
    (a read across an utterance's end would show as inf / nan in d'): bit-equal to itself alone and at another position of
    another batch, the same call twice bit-equal, and d' within the bound of the reference."""
    p = _pitch(sr, hop)
    F, W, tau_max = p.tile_frames, p.win_length, p.tau_max
    rng = np.random.default_rng(7)
    lens = [1, F * hop - 1, (3 * F + 1) * hop - 1, 77, F * hop, (2 * F - 1) * hop + 5]
    assert pr.n_frames(lens[0], hop) == 1 and pr.n_frames(lens[2], hop) == 3 * F + 1
    sig = pr.make_signal(sr, 4)
    xs = [(sig[:n] if k % 2 else rng.standard_normal(n).astype(np.float32)).copy() for k, n in enumerate(lens)]
    xs = [xs[i] for i in rng.permutation(len(xs))]
    guard = np.full(W + tau_max + 3, 1e30, np.float32)
    batch = [guard]
    for x in xs:
        batch += [x, guard]
    out = _run(p, batch)[1::2]
    again = _run(p, batch)[1::2]
    other = _run(p, xs[::-1])[::-1]
    eps = pr.eps_d(W, tau_max)
    worst = 0.0
    for x, a, b, c in zip(xs, out, again, other):
        alone = _run(p, [x])[0]
        assert np.all(np.isfinite(a[2]))
        assert _same(a, alone) and _same(b, alone) and _same(c, alone)
        want = pr.cmnd(x, hop, tau_max, W)
        worst = max(worst, fb.ratio(a[2], want, eps * np.abs(want)))
    print(f"pitch {sr}/{hop} ragged batch: d' ratio {worst:.4f}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------- lag and f0
@pytest.mark.parametrize("seconds", [pr.DUR, 0.4])
def test_lag_and_f0_on_decided_frames(seconds):
    sr, hop = 24000, 300
    p = _pitch(sr, hop)
    eps = pr.eps_d(p.win_length, p.tau_max)
    refs = [_ref(sr, hop, seed, seconds) for seed in (0, 1, 2)]
    got = _run(p, [x for x, _ in refs])
    worst = 0.0
    for seed, ((x, res), (f0, lag, cm)) in enumerate(zip(refs, got)):
        ok = pr.decided(res, eps)
        n = ok.size
        voiced = res["lag"] > 0
        assert (n - ok.sum()) <= 0.05 * n and (ok & voiced).sum() >= 0.40 * n
        assert np.array_equal(lag[ok], res["lag"][ok])
        assert np.all(f0[ok & ~voiced].view(np.uint32) == 0)          # unvoiced: exactly +0.0
        r = fb.ratio(f0, res["f0"], pr.f0_tolerance(res, sr, eps), where=ok)
        diff = np.abs(f0 - res["f0"])[ok & voiced].max()
        print(f"pitch seed {seed}, {seconds} s: {n} frames, {n - ok.sum()} undecided, {(ok & voiced).sum()} voiced and decided, "
              f"largest |f0 - ref| {diff:.3g} Hz, f0 ratio {r:.4f}, lags equal on undecided frames too: "
              f"{np.array_equal(lag, res['lag'])}")
        worst = max(worst, r)
    assert worst <= 1.0


# --------------------------------------------------------------------------------- continuous / log / token mean
def _golden_tracks():
    g = np.load(GOLDEN)
    rng = np.random.default_rng(3)
    tracks = [g[str(n) + "_f0"].astype(np.float32) for n in g["names"]]
    tracks.append(np.array([123.5], np.float32))                      # a single frame
    tracks.append(np.zeros(1, np.float32))
    long = np.where(rng.uniform(size=3 * 256 + 41) < 0.9, 0.0, rng.uniform(90, 380, 3 * 256 + 41)).astype(np.float32)
    long[250:530] = 0.0                                               # a gap that spans a whole scan chunk
    tracks.append(long)
    tracks.append(np.concatenate([np.zeros(300), [200.0], np.zeros(300)]).astype(np.float32))
    return tracks


def test_continuous_and_log_f0():
    from parakeet_amd.audio import continuous_f0_batch
    p = _pitch()
    tracks = _golden_tracks()
    r_cont = r_log = 0.0
    for use_log, outs in ((False, continuous_f0_batch(tracks)), (True, continuous_f0_batch(tracks, use_log_f0=True))):
        for f, o in zip(tracks, outs):
            o = o.cpu().numpy()
            want = pr.continuous_f0(f)
            nz = np.nonzero(f)[0]
            if nz.size == 0:
                assert np.array_equal(_bits(o), _bits(f))              # all unvoiced: as it came
                continue
            # every value lies between its voiced neighbours: the tolerance 4u max(|f(a)|, |f(b)|)
            prev = np.maximum.accumulate(np.where(f != 0, np.arange(f.size), -1))
            nxt = np.minimum.accumulate(np.where(f != 0, np.arange(f.size), f.size)[::-1])[::-1]
            fa, fbv = f[np.where(prev < 0, nz[0], prev)], f[np.where(nxt >= f.size, nz[-1], nxt)]
            tol = 4 * fb.U * np.maximum(np.abs(fa), np.abs(fbv)).astype(np.float64)
            if not use_log:
                r_cont = max(r_cont, fb.ratio(o, want, tol))
                assert np.array_equal(_bits(o[nz]), _bits(f[nz]))      # voiced frames pass through
            else:
                bound, usable = fb.log_bound(want, tol, 0.0, 1.0)
                assert usable.all()
                r_log = max(r_log, fb.ratio(o, np.log(want), bound))
    one = p._convert_to_continuous_f0(tracks[1]).cpu().numpy()
    assert np.array_equal(_bits(one), _bits(continuous_f0_batch(tracks)[1].cpu().numpy()))
    raw = continuous_f0_batch(tracks, use_log_f0=True, fill=False)     # the log step alone
    for f, o in zip(tracks, raw):
        o, nz = o.cpu().numpy(), f != 0
        want = np.log(f[nz].astype(np.float64))
        assert np.all(o[~nz] == 0) and fb.ratio(o[nz], want, 4 * fb.U * np.maximum(np.abs(want), 1.0)) <= 1.0
    print(f"continuous f0: ratio {r_cont:.4f}, log: ratio {r_log:.4f}")
    assert r_cont <= 1.0 and r_log <= 1.0


def test_get_pitch_and_its_batch():
    import torch
    from parakeet_amd.audio import average_by_duration
    p = _pitch()
    xs = [pr.make_signal(24000, 5, s) for s in (0.4, 0.25, 0.7)]
    durs = []
    for x in xs:
        n = pr.n_frames(x.size, 300)
        d = np.array([3, 0, 5, 0, 0, 4], dtype=np.int64)
        durs.append(np.concatenate([d, [n - d.sum()]]))
    batch = p.get_pitch_batch(xs, durs)
    worst = 0.0
    for x, d, b in zip(xs, durs, batch):
        f0 = p._calculate_f0(x)
        assert isinstance(f0, torch.Tensor) and f0.shape == (pr.n_frames(x.size, 300),)
        one = p.get_pitch(x, duration=d)
        assert one.shape == (d.size, 1)
        assert torch.equal(one, average_by_duration(f0, d).reshape(-1, 1))
        assert torch.equal(one, b)
        assert torch.equal(p.get_pitch(x), f0) and torch.equal(p.get_pitch(x, use_token_averaged_f0=False, duration=d), f0)
        # the token mean of the engine's own log f0: (n + 1) u mean|x| per token
        f64 = f0.cpu().numpy().astype(np.float64)
        cum = np.concatenate([[0], np.cumsum(d)])
        tol = np.array([(b_ - a_ + 1) * fb.U * np.abs(f64[a_:b_]).mean() if b_ > a_ else 0.0 for a_, b_ in zip(cum[:-1], cum[1:])])
        worst = max(worst, fb.ratio(one.cpu().numpy(), pr.average(f64, d), tol.reshape(-1, 1)))
    raw = [a.cpu().numpy() for a, _ in p.track(xs)]
    plain = p.get_pitch_batch(xs, None, use_continuous_f0=False, use_log_f0=False)
    assert all(np.array_equal(_bits(a), _bits(b.cpu().numpy())) for a, b in zip(raw, plain))
    print(f"token-averaged pitch: ratio {worst:.4f}")
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_refusals():
    from parakeet_amd import _capi
    from parakeet_amd.runtime import Context, dptr
    ctx = Context.get()
    lib = ctx.lib
    h = C.c_void_p()
    for cfg, word in (((24000, 300, 60, 961, 1922, 0.1), "960"), ((24000, 300, 60, 300, 601, 0.1), "600"),
                      ((24000, 300, 1, 300, 600, 0.1), "tau_min"), ((24000, 300, 299, 300, 600, 0.1), "tau_min"),
                      ((24000, 16385, 60, 300, 600, 0.1), "16384")):
        c = _capi.PitchCfg(*cfg)
        assert lib.pk_pitch_create(ctx.handle, C.byref(c), C.byref(h)) == -3
        assert word in lib.pk_last_error().decode() and not h.value
    c = _capi.PitchCfg(24000, 300, 60, 300, 600, 0.1)
    assert lib.pk_pitch_create(ctx.handle, None, C.byref(h)) == -1
    assert lib.pk_pitch_create(None, C.byref(c), C.byref(h)) == -1
    p = _pitch()
    x = ctx.to_device(pr.make_signal(24000, 0, 0.05))
    n = x.numel()
    nf = C.c_int32()
    assert lib.pk_pitch_frames(p.h, n, C.byref(nf)) == 0 and nf.value == n // 300 + 1
    assert lib.pk_pitch_frames(p.h, -1, C.byref(nf)) == -1
    assert lib.pk_pitch_frames(None, n, C.byref(nf)) == -1
    f0, f0b = ctx.empty((nf.value,)), ctx.empty((nf.value,))
    lens = (C.c_int32 * 2)(n, 0)
    run = lib.pk_pitch_run
    assert run(None, dptr(x), lens, 1, dptr(f0), None, None, 0) == -1
    assert run(p.h, None, lens, 1, dptr(f0), None, None, 0) == -1
    assert run(p.h, dptr(x), None, 1, dptr(f0), None, None, 0) == -1
    assert run(p.h, dptr(x), lens, 1, None, None, None, 0) == -1
    assert run(p.h, dptr(x), lens, 0, dptr(f0), None, None, 0) == -1
    assert run(p.h, dptr(x), lens, 2, dptr(f0), None, None, 0) == -1 and b"empty" in lib.pk_last_error()
    _capi.check(run(p.h, dptr(x), lens, 1, dptr(f0), None, None, 0))           # lag_out and cmnd_out may be NULL
    want = p.track([x])[0][0]
    assert np.array_equal(_bits(f0.cpu().numpy()), _bits(want.cpu().numpy()))
    # host pointers give what device pointers give
    xh = x.cpu().numpy()
    fh, lh = np.empty(nf.value, np.float32), np.empty(nf.value, np.int32)
    _capi.check(run(p.h, _capi.fptr(xh), lens, 1, _capi.fptr(fh), lh.ctypes.data_as(C.c_void_p), None, _capi.PK_HOST_IO))
    assert np.array_equal(_bits(fh), _bits(want.cpu().numpy())) and np.array_equal(lh, p.track([x])[0][1].cpu().numpy())
    cont = lib.pk_op_continuous_f0
    fr = (C.c_int32 * 2)(nf.value, 0)
    assert cont(ctx.handle, None, fr, 1, 0, dptr(f0b)) == -1
    assert cont(ctx.handle, dptr(f0), None, 1, 0, dptr(f0b)) == -1
    assert cont(ctx.handle, dptr(f0), fr, 1, 0, None) == -1
    assert cont(ctx.handle, dptr(f0), fr, 0, 0, dptr(f0b)) == -1
    assert cont(ctx.handle, dptr(f0), fr, 2, 0, dptr(f0b)) == -1 and b"empty" in lib.pk_last_error()
    _capi.check(cont(ctx.handle, dptr(f0), fr, 1, 0, dptr(f0b)))
    assert np.array_equal(_bits(f0b.cpu().numpy()), _bits(p._convert_to_continuous_f0(f0).cpu().numpy()))


# ---------------------------------------------------------------------------------------------------------- example
def _load_example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_fastspeech2_features(tmp_path):
    import yaml
    from parakeet_amd.audio import write_wav
    cfg = dict(fs=24000, n_fft=2048, n_shift=300, win_length=1200, window="hann", n_mels=80, fmin=80, fmax=7600, f0min=80,
               f0max=400)
    (tmp_path / "conf.yaml").write_text(yaml.safe_dump(cfg))
    (tmp_path / "wav").mkdir()
    lines, want = [], {}
    for k, (utt, sr, secs) in enumerate((("a", 24000, 0.5), ("b", 48000, 0.4), ("c", 24000, 0.3))):
        write_wav(tmp_path / "wav" / (utt + ".wav"), pr.make_signal(sr, 10 + k, secs), sr, subtype="FLOAT")
        frames = int(secs * 24000) // 300 + 1
        durs = [4, frames - 12 + k, 5, 3]                             # sums to frames + k - ... : fixed up by the script
        phones = ["sil", "a1", "b2", "sil"]
        lines.append(f"{utt}|spk{k % 2}|" + " ".join(f"{p} {d}" for p, d in zip(phones, durs)))
        want[utt] = (phones, durs, frames)
    (tmp_path / "durations.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "phones.txt").write_text("sil 1\na1 2\nb2 3\n")
    mod = _load_example("fastspeech2_features")
    args = mod.parse_args(["--config", str(tmp_path / "conf.yaml"), "--input-dir", str(tmp_path / "wav"), "--durations",
                           str(tmp_path / "durations.txt"), "--output-dir", str(tmp_path / "dump"), "--phones-dict",
                           str(tmp_path / "phones.txt")])
    recs = mod.extract(args)
    assert [r["utt_id"] for r in recs] == ["a", "b", "c"]
    items = _load_example("fastspeech2_gta").read_metadata(str(tmp_path / "dump" / "metadata.jsonl"))
    assert len(items) == 3
    for it in items:
        phones, durs, frames = want[it["utt_id"]]
        assert it["durations"].sum() == frames and list(it["text"]) == [1, 2, 3, 1]
        assert np.load(it["feats"]).shape == (frames, 80)
        assert np.load(it["pitch"]).shape == np.load(it["energy"]).shape == (4, 1)
        assert np.load(it["pitch"]).dtype == np.float32 and np.isfinite(np.load(it["pitch"])).all()
    assert len([json.loads(s) for s in (tmp_path / "dump" / "metadata.jsonl").read_text().splitlines()]) == 3
    # --cut-sil and statistics: the sil tokens and their samples go, the features are z-scored
    np.save(tmp_path / "ps.npy", np.array([[5.0], [0.5]]))
    args = mod.parse_args(["--config", str(tmp_path / "conf.yaml"), "--input-dir", str(tmp_path / "wav"), "--durations",
                           str(tmp_path / "durations.txt"), "--output-dir", str(tmp_path / "dump2"), "--cut-sil",
                           "--pitch-stats", str(tmp_path / "ps.npy")])
    recs2 = mod.extract(args)
    a = recs2[0]
    assert a["phones"] == ["a1", "b2"] and np.load(tmp_path / "dump2" / a["pitch"]).shape == (2, 1)
    assert sum(a["durations"]) == np.load(tmp_path / "dump2" / a["feats"]).shape[0]
