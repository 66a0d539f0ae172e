"""FastSpeech2 with given durations, pitch and energy on the engine: ``forward``, ``teacher_forced_batch``,
``inference(use_teacher_forcing=True)``, ``predict_batch`` and the overrides of ``inference_batch``; ``audio.Energy`` and
``audio.average_by_duration``; examples/fastspeech2_gta.py.

Bars: the golden vectors of the reference's own source (golden/fs2_forward.npz) under the figures tests/test_fs2_gpu.py
applies to the same quantities; the fp64 restatement (tests/fs2_forward_ref.py) at recipe size under that file's
f32 / f16x3 bars; bit equality wherever two calls compute the same thing.  The Energy bound is derived below from
tests/fp32_bounds.py, not tuned.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp32_bounds as fb  # noqa: E402
import fs2_forward_cases as cases  # noqa: E402
import fs2_forward_ref as fref  # noqa: E402
import sweep_cases as sc  # noqa: E402
from parakeet_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fs2_forward.npz")
MEL_L1_TOL = 1e-4      # tests/test_fs2_gpu.py:16-17
MEL_MAX_TOL = 2e-3
PRED_TOL = 1e-3        # tests/test_fs2_gpu.py:59-61 (pitch / energy taps)
MATHS = ("f32", "f16x3")


def _t(x):
    return x.as_subclass(torch.Tensor).detach().cpu()


def _case_model(name):
    from parakeet_amd.fastspeech2 import FastSpeech2
    m = FastSpeech2(80, 80, **cases.model_kwargs(name))
    m.set_state_dict(cases.case_state(name))
    m.eval()
    return m


def _ljspeech_model(seed=150):
    from parakeet_amd.fastspeech2 import FastSpeech2
    cfg = dict(syn.FS2_LJSPEECH)
    m = FastSpeech2(80, 80, **cfg)
    m.set_state_dict(syn.fastspeech2_state(80, 80, cfg, seed=seed))
    m.eval()
    return m


def _padded(utts, r=1):
    """The padded batch forward() takes, from per-utterance arrays."""
    B, Tmax = len(utts), max(len(u["ids"]) for u in utts)
    text, ds = np.zeros((B, Tmax), np.int64), np.zeros((B, Tmax), np.int64)
    ps, es = np.zeros((B, Tmax, 1), np.float32), np.zeros((B, Tmax, 1), np.float32)
    for b, u in enumerate(utts):
        T = len(u["ids"])
        text[b, :T], ds[b, :T], ps[b, :T, 0], es[b, :T, 0] = u["ids"], u["ds"], u["ps"], u["es"]
    olens = np.array([u.get("olen", r * int(u["ds"].sum())) for u in utts], np.int64)
    speech = np.zeros((B, int(olens.max()), 80), np.float32)
    return dict(text=text, text_lengths=np.array([len(u["ids"]) for u in utts], np.int64), speech=speech,
                speech_lengths=olens, durations=ds, pitch=ps, energy=es)


def _assert_mel(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)       # lengths: exact
    if got.size:
        l1, mx = float(np.abs(got - want).mean()), float(np.abs(got - want).max())
        print(f"FS2-FORWARD {what} L1 {l1:.3g} max {mx:.3g}")
        assert l1 < MEL_L1_TOL and mx < MEL_MAX_TOL, (what, l1, mx)


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", list(cases.CASES))
def test_against_reference_source(name, math):
    g = np.load(GOLD)
    _, how, _, spk = cases.CASES[name]
    m = _case_model(name)
    m.set_math(math)
    utts = cases.case_inputs(name)
    r = m.reduction_factor
    kw = {}
    if spk == "spk_id":
        kw["spk_id"] = np.array([u["spk_id"] for u in utts], np.int64)
    elif spk == "spembs":
        kw["spembs"] = np.stack([u["spembs"] for u in utts])
    if how == "inference":
        u = utts[0]
        mel = m.inference(u["ids"], durations=u["ds"], pitch=u["ps"][:, None], energy=u["es"][:, None],
                          use_teacher_forcing=True)
        _assert_mel(mel.numpy(), g[f"{name}_after0"], f"{name} {math} after")
        return
    if how == "forward":
        before, after, d, p, e, ys, olens = m.forward(**_padded(utts, r), **kw)
        assert [int(v) for v in olens] == [int(v) for v in g[f"{name}_olens_out"]]
        assert ys.shape[1] == int(g[f"{name}_ys_len"])
        before, after, d, p, e = _t(before).numpy(), _t(after).numpy(), _t(d).numpy(), _t(p).numpy()[:, :, 0], _t(e).numpy()[:, :, 0]
        per = [(before[b, :r * int(u["ds"].sum())], after[b, :r * int(u["ds"].sum())], d[b], p[b], e[b])
               for b, u in enumerate(utts)]
        assert before.shape[1] == max(r * int(u["ds"].sum()) for u in utts)
    else:
        outs = m.teacher_forced_batch([u["ids"] for u in utts], [u["ds"] for u in utts], [u["ps"] for u in utts],
                                      [u["es"] for u in utts], spk_ids=kw.get("spk_id"), spembs=kw.get("spembs"),
                                      return_before=True)
        d, p, e = m.read_predictions()
        per = [(bo.numpy(), ao.numpy(), d[b], p[b], e[b]) for b, (bo, ao) in enumerate(outs)]
    for b, (bo, ao, db, pb, eb) in enumerate(per):
        _assert_mel(ao, g[f"{name}_after{b}"], f"{name}[{b}] {math} after")
        _assert_mel(bo, g[f"{name}_before{b}"], f"{name}[{b}] {math} before")
        for k, v in (("d_outs", db), ("p_outs", pb), ("e_outs", eb)):
            want = g[f"{name}_{k}{b}"]
            assert v.shape == want.shape, (name, k)
            err = float(np.abs(v - want).max())
            print(f"FS2-FORWARD {name}[{b}] {math} {k} max {err:.3g}")
            assert err < PRED_TOL, (name, k, err)


def _ragged_targets(tok_lens, seed):
    rng = np.random.default_rng(seed)
    utts = []
    for i, T in enumerate(tok_lens):
        utts.append(dict(ids=syn.phoneme_ids(T, 80, seed=seed + 10 + i), ds=rng.integers(0, 10, size=T).astype(np.int64),
                         ps=rng.normal(size=T).astype(np.float32), es=rng.normal(size=T).astype(np.float32)))
    return utts


def test_against_fp64_restatement_at_recipe_size():
    """LJSpeech configuration, ragged T in 37 .. 128, random durations 0 .. 9: f32 L1 < 2e-5 and f16x3 < 2 * f32 + 5e-7 per
    utterance (tests/test_fs2_gpu.py:144-145), on after_outs and before_outs."""
    cfg = dict(syn.FS2_LJSPEECH)
    state = syn.fastspeech2_state(80, 80, cfg, seed=160)
    utts = _ragged_targets([37, 128, 64, 91], seed=161)
    m = _ljspeech_model(160)
    want = [fref.forward(state, u["ids"], u["ds"], u["ps"], u["es"], cfg, dtype=torch.float64) for u in utts]
    l1 = {}
    for math in MATHS:
        m.set_math(math)
        outs = m.teacher_forced_batch([u["ids"] for u in utts], [u["ds"] for u in utts], [u["ps"] for u in utts],
                                      [u["es"] for u in utts], return_before=True)
        d, p, e = m.read_predictions()
        for b, (bo, ao) in enumerate(outs):
            assert ao.shape == want[b]["after"].shape == (int(utts[b]["ds"].sum()), 80)
            l1[math, b, "after"] = float(np.abs(ao.numpy() - want[b]["after"].numpy()).mean())
            l1[math, b, "before"] = float(np.abs(bo.numpy() - want[b]["before"].numpy()).mean())
            for k, v in (("d_outs", d[b]), ("p_outs", p[b]), ("e_outs", e[b])):
                assert np.abs(v - want[b][k].numpy()).max() < PRED_TOL, (math, b, k)
    for k, v in l1.items():
        print("FS2-FORWARD fp64", k, f"{v:.3g}")
    for b in range(len(utts)):
        for what in ("after", "before"):
            assert l1["f32", b, what] < 2e-5, (b, what, l1["f32", b, what])
            assert l1["f16x3", b, what] < 2.0 * l1["f32", b, what] + 5e-7, (b, what, l1["f16x3", b, what], l1["f32", b, what])


TEXT_LENS = [37, 5, 64, 1, 23]


def _texts(seed=151):
    return [syn.phoneme_ids(T, 80, seed=seed + i) for i, T in enumerate(TEXT_LENS)]


@pytest.mark.parametrize("alpha", [1.0, 1.3])
def test_round_trip_is_bit_exact(alpha):
    """predict_batch -> inference_batch(durations=, pitch=, energy=) equals plain inference_batch exactly: all three fed
    back, and each alone.  The returned durations carry alpha, and alpha does not scale given durations."""
    m = _ljspeech_model()
    texts = _texts()
    plain = [_t(o).clone() for o in m.inference_batch(texts, alpha=alpha)]
    pred = m.predict_batch(texts, alpha=alpha)
    assert all(d.dtype == np.int64 and d.shape == p.shape == e.shape == (T,) for (d, p, e), T in zip(pred, TEXT_LENS))
    assert [int(d.sum()) for d, _, _ in pred] == [o.shape[0] for o in plain]
    ds, ps, es = [x[0] for x in pred], [x[1] for x in pred], [x[2] for x in pred]
    for kw in (dict(durations=ds, pitch=ps, energy=es), dict(durations=ds), dict(pitch=ps), dict(energy=es)):
        again = m.inference_batch(texts, alpha=alpha, **kw)
        for b in range(len(texts)):
            assert torch.equal(plain[b], _t(again[b])), (sorted(kw), b)


def test_forward_equals_each_utterance_alone_and_inference():
    m = _ljspeech_model()
    utts = _ragged_targets(TEXT_LENS, seed=170)
    out = m.forward(**_padded(utts))
    again = m.forward(**_padded(utts))
    for a, b in zip(out[:5], again[:5]):                    # the same call twice
        assert torch.equal(_t(a), _t(b))
    before, after, d, p, e = (_t(x) for x in out[:5])
    assert [int(v) for v in out[6]] == [int(u["ds"].sum()) for u in utts]
    for b, u in enumerate(utts):
        L, T = int(u["ds"].sum()), len(u["ids"])
        solo = m.forward(**_padded([u]))
        sb, sa, sd, sp, se = (_t(x) for x in solo[:5])
        assert sa.shape == (1, L, 80)
        assert torch.equal(after[b, :L], sa[0]) and torch.equal(before[b, :L], sb[0]), b
        assert torch.equal(d[b, :T], sd[0]) and torch.equal(p[b, :T], sp[0]) and torch.equal(e[b, :T], se[0]), b
        assert not after[b, L:].any() and not before[b, L:].any() and not d[b, T:].any() and not p[b, T:].any()
        mel = m.inference(u["ids"], durations=u["ds"], pitch=u["ps"], energy=u["es"], use_teacher_forcing=True)
        assert torch.equal(_t(mel), sa[0]), b               # forward with B = 1 == inference(use_teacher_forcing=True)
        mel2 = m.inference(u["ids"], durations=u["ds"], pitch=u["ps"][:, None], energy=u["es"][:, None],
                           use_teacher_forcing=True, alpha=1.7)     # (T, 1) targets; alpha is not applied
        assert torch.equal(_t(mel2), sa[0]), b


def test_targets_are_consumed_and_ignored_without_the_switch():
    m = _ljspeech_model()
    u = _ragged_targets([23], seed=171)[0]
    first = _t(m.inference(u["ids"])).clone()
    forced = _t(m.inference(u["ids"], durations=u["ds"], pitch=u["ps"], energy=u["es"], use_teacher_forcing=True))
    assert forced.shape[0] == int(u["ds"].sum())
    assert torch.equal(first, _t(m.inference(u["ids"])))                                    # the setting did not stay
    assert torch.equal(first, _t(m.inference(u["ids"], durations=u["ds"], pitch=u["ps"], energy=u["es"])))   # ignored


def test_control_changes_what_it_should():
    m = _ljspeech_model()
    texts = _texts()
    pred = m.predict_batch(texts)
    ds, ps, es = [x[0] for x in pred], [x[1] for x in pred], [x[2] for x in pred]
    base = [_t(o).clone() for o in m.inference_batch(texts, durations=ds, pitch=ps, energy=es)]
    b = 2
    k = int(np.argmax(ds[b] > 0))
    assert ds[b][k] > 0
    longer = [d.copy() for d in ds]
    longer[b][k] *= 2
    out = m.inference_batch(texts, durations=longer)
    for i in range(len(texts)):
        assert out[i].shape[0] == base[i].shape[0] + (int(ds[b][k]) if i == b else 0)
        if i != b:
            assert torch.equal(_t(out[i]), base[i])
    m.inference_batch(texts, pitch=ps)
    d0, p0, e0 = m.read_predictions()
    raised = m.inference_batch(texts, pitch=[p + np.float32(1.0) for p in ps])
    d1, p1, e1 = m.read_predictions()
    for i in range(len(texts)):
        assert raised[i].shape == base[i].shape
        assert np.abs(raised[i].numpy() - base[i].numpy()).max() > 1e-3, i
        assert np.array_equal(d0[i], d1[i]) and np.array_equal(e0[i], e1[i]) and np.array_equal(p0[i], p1[i])
        assert np.array_equal(d1[i].astype(np.int64), ds[i])


def test_refusals_leave_the_handle_usable():
    from parakeet_amd import _capi
    m = _ljspeech_model()
    utts = _ragged_targets([9, 4], seed=172)
    texts = [u["ids"] for u in utts]
    good = [_t(o).clone() for o in m.inference_batch(texts)]
    n = sum(len(t) for t in texts)
    d = np.ascontiguousarray(np.concatenate([u["ds"] for u in utts] + [np.array([1], np.int64)]))
    _capi.check(m._ctx.lib.pk_fs2_set_targets(m._h, d.ctypes.data_as(C.POINTER(C.c_int64)), None, None, n + 1))
    with pytest.raises(AssertionError):                     # PK_ESHAPE: n differs from the call's token total
        m.encode_batch(texts)
    for a, b in zip(good, m.inference_batch(texts)):        # ... and the refused setting is gone
        assert torch.equal(a, _t(b))
    with pytest.raises(ValueError):                         # PK_EINVAL: negative duration
        m.inference_batch(texts, durations=[np.array([1, -1] + [1] * 7), utts[1]["ds"]])
    with pytest.raises(ValueError):                         # one value per token
        m.inference_batch(texts, pitch=[utts[0]["ps"][:-1], utts[1]["ps"]])
    bad = _padded(utts)
    bad["speech_lengths"] = bad["speech_lengths"] + np.array([0, 1])
    with pytest.raises(ValueError):                         # speech_lengths // r != sum of durations
        m.forward(**bad)
    with pytest.raises(ValueError):                         # a missing target under use_teacher_forcing
        m.inference(texts[0], durations=utts[0]["ds"], pitch=utts[0]["ps"], use_teacher_forcing=True)
    with pytest.raises(NotImplementedError, match="TIME axis"):
        m.forward(**_padded(utts), tone_id=np.zeros((2, 9), np.int64))
    with pytest.raises(AssertionError):                     # the whole-batch readout checks its size
        m.encode_batch(texts)
        out = np.empty(n + 1, np.float32)
        _capi.check(m._ctx.lib.pk_fs2_read_predictions(m._h, _capi.fptr(out), None, None, n + 1))
    for a, b in zip(good, m.inference_batch(texts)):
        assert torch.equal(a, _t(b))


def test_all_zero_durations_give_an_empty_mel():
    m = _ljspeech_model()
    utts = _ragged_targets([6, 3], seed=173)
    utts[1]["ds"][:] = 0
    outs = m.teacher_forced_batch([u["ids"] for u in utts], [u["ds"] for u in utts], [u["ps"] for u in utts],
                                  [u["es"] for u in utts], return_before=True)
    assert outs[1][0].shape == outs[1][1].shape == (0, 80)
    solo = m.teacher_forced_batch([utts[0]["ids"]], [utts[0]["ds"]], [utts[0]["ps"]], [utts[0]["es"]])[0]
    assert torch.equal(_t(outs[0][1]), _t(solo))


# ------------------------------------------------------------------------------------------------ Energy
def _energy_reference(c, wav):
    """fp64 energy of one utterance and its bound.  S = sum_k p_k, p_k = re_k^2 + im_k^2, E = sqrt(max(S, floor)).
    * p_k: fb.power_bound from the STFT product's dot bound, b_p;
    * the sum of n_bin non-negative terms in any order adds gamma_(n_bin) * (S + sum b_p) (Higham (4.4); n_bin rather than
      n_bin - 1: the kernel may or may not contract re*re + im*im + s, one spare rounding);
    * max(., floor) is 1-Lipschitz; |sqrt(a') - sqrt(a)| = |a' - a| / (sqrt(a') + sqrt(a)) <= b_S / sqrt(a) with
      a = max(S, floor) > 0;
    * sqrtf: 2u relative (one spare ulp, as fb.magnitude_bound)."""
    basis = np.zeros((1, 1 + c.n_fft // 2), np.float32)
    r = sc.mel_reference(c, wav, basis, power=True)
    nb = 1 + c.n_fft // 2
    re, im, b_re, b_im = r["reim"][:, :nb], r["reim"][:, nb:], r["b_reim"][:, :nb], r["b_reim"][:, nb:]
    p = re * re + im * im
    b_p = fb.power_bound(re, im, b_re, b_im)
    S = p.sum(axis=1)
    gamma = nb * fb.U / (1.0 - nb * fb.U)
    b_S = b_p.sum(axis=1) + gamma * (S + b_p.sum(axis=1))
    a = np.maximum(S, sc.MEL_FLOOR)
    E = np.sqrt(a)
    b_sqrt = b_S / np.sqrt(a)
    return E, b_sqrt + 2.0 * fb.U * (E + b_sqrt)


@pytest.mark.parametrize("c", sc.MEL_CFGS, ids=sc.mel_id)
def test_energy_against_fp64_stft(c):
    from parakeet_amd import _capi
    from parakeet_amd.audio import _Engine
    eng = _Engine(c.n_fft, c.hop, c.win, "hann", c.center, False, None, 0)
    wavs = sc.mel_batch(c)
    got = [o.detach().cpu().numpy() for o in eng.run(wavs, 3)]
    worst = 0.0
    for u, w in enumerate(wavs):
        F = sc.num_frames(c, len(w))
        assert got[u].shape == (F, 1)
        if F == 0:
            continue
        E, bound = _energy_reference(c, w)
        worst = max(worst, fb.ratio(got[u][:, 0], E, bound))
        assert np.array_equal(eng.run([w], 3)[0].detach().cpu().numpy(), got[u]), u      # alone == in the batch
    print(f"SWEEP-RATIO energy {sc.mel_id(c)} {worst:.4g}")
    assert worst <= 1.0
    # silence: the clip certainly acts, every frame is sqrt(floor) up to the rounding of sqrtf
    assert np.array_equal(got[1], np.full_like(got[1], got[1][0, 0]))
    assert abs(float(got[1][0, 0]) - np.sqrt(sc.MEL_FLOOR)) <= 2.0 * fb.U * np.sqrt(sc.MEL_FLOOR)
    lens = np.array([len(w) for w in wavs], dtype=np.int32)
    x = np.ascontiguousarray(np.concatenate(wavs), dtype=np.float32)
    host = np.full((sum(g.shape[0] for g in got), 1), np.nan, np.float32)
    _capi.check(eng.ctx.lib.pk_mel_run(eng.h, _capi.fptr(x), lens.ctypes.data_as(C.POINTER(C.c_int32)), len(wavs),
                                       _capi.fptr(host), 3, _capi.PK_HOST_IO))
    assert np.array_equal(host, np.concatenate(got))


def test_energy_class_and_average_by_duration():
    from parakeet_amd.audio import Energy, average_by_duration, average_by_duration_numpy
    c = sc.MEL_CFGS[1]                                       # the FastSpeech2 recipes' analysis: 24 kHz, 2048 / 300 / 1200
    en = Energy(sr=c.sr, n_fft=c.n_fft, hop_length=c.hop, win_length=c.win)
    wav = sc.mel_batch(c)[-1]
    e = en.get_energy(wav, duration=None)
    E, bound = _energy_reference(c, wav)
    assert e.shape == E.shape and fb.ratio(e.numpy(), E, bound) <= 1.0
    F = E.shape[0]
    rng = np.random.default_rng(8)
    # mean of n fp32 values in any order: gamma_(n - 1) * sum|x| / n, plus the rounding of the quotient: (n + 1) u mean|x|
    for d in ([0, 3, 0, 0, F - 10, 7, 0], [F], [1] * 5 + [0] + [F - 5], [F - 20, 40], [5, 5]):
        d = np.array(d, np.int64)
        for x in (e.numpy(), rng.normal(size=(F, 3)).astype(np.float32)):
            got = average_by_duration(x, d).numpy()
            want = average_by_duration_numpy(x.astype(np.float64), d)
            absmean = average_by_duration_numpy(np.abs(x).astype(np.float64), d)
            cum = np.minimum(np.concatenate([[0], np.cumsum(d)]), F)
            n = (cum[1:] - cum[:-1]).reshape((-1,) + (1,) * (x.ndim - 1))
            assert got.shape == want.shape == (len(d),) + x.shape[1:]
            assert fb.ratio(got, want, (n + 1) * fb.U * absmean) <= 1.0
            assert not got[n.reshape(-1) == 0].any()
    d = np.array([0, 3, 0, 0, F - 10, 7, 0], np.int64)
    tok = en.get_energy(wav, duration=d)
    assert tok.shape == (len(d), 1)
    assert np.array_equal(tok.numpy()[:, 0], average_by_duration(e, d).numpy())
    with pytest.raises(ValueError):
        average_by_duration(e, np.array([1, -1]))


def test_analysis_pass_feeds_teacher_forcing():
    """wav -> LogMelFBank + Energy -> token averages -> teacher_forced_batch: frame counts agree along the way, and the
    device tensors the feature side returns are accepted as targets and give what their host copies give."""
    from parakeet_amd.audio import Energy, LogMelFBank, average_by_duration
    rng = np.random.default_rng(12)
    fbank, en = LogMelFBank(sr=24000, n_fft=2048, hop_length=300, win_length=1200), Energy(24000, 2048, 300, 1200)
    m = _ljspeech_model()
    texts, ds, ps, es, frames = [], [], [], [], []
    for i, T in enumerate([11, 6]):
        wav = np.clip(rng.normal(0.0, 0.2, 300 * (20 + 9 * i) + 57), -1, 1).astype(np.float32)
        mel = fbank.get_log_mel_fbank(wav)
        energy = en.get_energy(wav, duration=None)
        assert mel.shape == (energy.shape[0], 80)
        F = mel.shape[0]
        d = rng.multinomial(F, np.ones(T) / T).astype(np.int64)
        f0 = rng.uniform(4.0, 6.0, size=F).astype(np.float32)            # callers bring frame-level f0
        texts.append(syn.phoneme_ids(T, 80, seed=300 + i))
        ds.append(d)
        ps.append(average_by_duration(f0, d))
        es.append(en.get_energy(wav, duration=d))
        frames.append(F)
        assert es[-1].shape == (T, 1) and ps[-1].shape == (T,)
    outs = m.teacher_forced_batch(texts, ds, ps, es)
    host = m.teacher_forced_batch(texts, ds, [p.numpy() for p in ps], [e.numpy() for e in es])
    for b in range(2):
        assert outs[b].shape == (frames[b], 80) and bool(torch.isfinite(_t(outs[b])).all())
        assert torch.equal(_t(outs[b]), _t(host[b]))


def test_gta_example(tmp_path):
    import pickle
    import yaml
    cfg = dict(syn.FS2_LJSPEECH, elayers=1, dlayers=1, postnet_layers=2)
    state = syn.fastspeech2_state(40, 80, cfg, seed=81)
    ckpt = tmp_path / "snapshot.pdz"
    with open(ckpt, "wb") as f:
        pickle.dump({"main_params": {k: ("t", v) for k, v in state.items()}}, f, protocol=2)
    conf = tmp_path / "default.yaml"
    conf.write_text(yaml.safe_dump({"fs": 24000, "n_mels": 80, "model": dict(cfg)}))
    stats = tmp_path / "speech_stats.npy"
    np.save(str(stats), np.stack([np.full(80, -4.0, np.float32), np.full(80, 0.5, np.float32)]))
    phones = tmp_path / "phone_id_map.txt"
    phones.write_text("".join(f"P{i} {i}\n" for i in range(40)))
    rng = np.random.default_rng(6)
    items = []
    for i, T in enumerate([5, 12, 3, 9, 12, 1]):
        d = rng.integers(0, 6, size=T)
        d[0] = max(int(d[0]), 1)
        for k in ("pitch", "energy"):
            np.save(str(tmp_path / f"u{i}_{k}.npy"), rng.normal(size=(T, 1)).astype(np.float32))
        it = dict(utt_id=f"u{i}", text_lengths=T, speech_lengths=int(d.sum()), durations=[int(v) for v in d],
                  pitch=str(tmp_path / f"u{i}_pitch.npy"), energy=f"u{i}_energy.npy")     # absolute and relative paths
        ids = [int(v) for v in syn.phoneme_ids(T, idim=40, seed=i)]
        if i % 2:
            it["phones"] = [f"P{v}" for v in ids]
        else:
            it["text"] = ids
        items.append((it, np.array(ids)))
    meta = tmp_path / "metadata.jsonl"
    meta.write_text("".join(json.dumps(it) + "\n" for it, _ in items))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fastspeech2_gta.py"),
                        "--fastspeech2-config", str(conf), "--fastspeech2-checkpoint", str(ckpt),
                        "--fastspeech2-stat", str(stats), "--phones-dict", str(phones), "--test-metadata", str(meta),
                        "--output-dir", str(out), "--batch-size", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    from parakeet_amd.fastspeech2 import FastSpeech2
    m = FastSpeech2(40, 80, **cfg)
    m.set_state_dict(state)
    m.eval()
    for it, ids in items:
        gta = np.load(str(out / f"{it['utt_id']}_gta.npy"))
        mel = m.teacher_forced_batch([ids], [np.array(it["durations"])], [np.load(str(tmp_path / f"{it['utt_id']}_pitch.npy"))],
                                     [np.load(str(tmp_path / f"{it['utt_id']}_energy.npy"))])[0]
        assert gta.shape == (sum(it["durations"]), 80)
        assert np.array_equal(gta, mel.numpy()), it["utt_id"]
