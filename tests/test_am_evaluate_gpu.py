"""``evaluate_batch`` / ``evaluate_per_utterance`` of FastSpeech2, TransformerTTS and Tacotron2 and ``TransformerTTS.forward``
on the engine, with the small seeded models of the forward tests (tests/fs2_forward_cases.py, tests/taco2_forward_cases.py,
tests/tts_teacher_ref.py).

Against the CPU oracle's forward no constant is introduced: a mean absolute error is a norm, so
|l1(engine) - l1(oracle)| <= mean |mel(engine) - mel(oracle)| (summed over before and after where the criterion sums
both); a mean squared error is a squared norm, so |sqrt(mse(engine)) - sqrt(mse(oracle))| <= rms(mel(engine) -
mel(oracle)).  Both sides are formed in the test from the two forwards."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import am_loss_ref as ar  # noqa: E402
import fs2_forward_cases as fcases  # noqa: E402
import fs2_forward_ref as fref  # noqa: E402
import taco2_forward_ref as tref  # noqa: E402
import tts_teacher_ref as ttr  # noqa: E402
from ar_cases import T2_CASES  # noqa: E402
from parakeet_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _np(t):
    return t.as_subclass(torch.Tensor).detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _rel(got, want, tol=1e-12):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in got:
        assert abs(got[k] - want[k]) <= tol * abs(want[k]), (k, got[k], want[k])


# ------------------------------------------------------------------------------------------------------------ FastSpeech2
def _fs2():
    from parakeet_amd.fastspeech2 import FastSpeech2
    m = FastSpeech2(80, 80, **fcases.model_kwargs("t7"))
    state = fcases.case_state("t7")
    m.set_state_dict(state)
    rng = np.random.default_rng(71)
    utts = []
    for b, T in enumerate((7, 3, 5)):
        ds = rng.integers(0, 5, size=T).astype(np.int64)
        ds[0] = max(int(ds[0]), 1)
        utts.append(dict(ids=syn.phoneme_ids(T, 80, seed=600 + b), ds=ds, ps=rng.normal(size=T).astype(np.float32),
                         es=rng.normal(size=T).astype(np.float32),
                         mel=rng.standard_normal((int(ds.sum()), 80)).astype(np.float32)))
    return m.eval(), state, utts


def _fs2_padded(utts):
    B, T, L = len(utts), max(len(u["ids"]) for u in utts), max(len(u["mel"]) for u in utts)
    x = dict(text=np.zeros((B, T), np.int64), text_lengths=np.array([len(u["ids"]) for u in utts]),
             speech=np.zeros((B, L, 80), np.float32), speech_lengths=np.array([len(u["mel"]) for u in utts]),
             durations=np.zeros((B, T), np.int64), pitch=np.zeros((B, T, 1), np.float32), energy=np.zeros((B, T, 1), np.float32))
    for b, u in enumerate(utts):
        n = len(u["ids"])
        x["text"][b, :n], x["durations"][b, :n], x["pitch"][b, :n, 0], x["energy"][b, :n, 0] = u["ids"], u["ds"], u["ps"], u["es"]
        x["speech"][b, :len(u["mel"])] = u["mel"]
    return x


def _fs2_args(utts):
    return ([u["ids"] for u in utts], [u["ds"] for u in utts], [u["ps"] for u in utts], [u["es"] for u in utts],
            [u["mel"] for u in utts])


@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True)])
def test_fastspeech2_evaluate_batch_is_forward_then_the_criterion(flags):
    from parakeet_amd.fastspeech2 import FastSpeech2Loss
    m, _, utts = _fs2()
    x = _fs2_padded(utts)
    got = m.evaluate_batch(**x, use_masking=flags[0], use_weighted_masking=flags[1])
    before, after, d, p, e, ys, olens = m.forward(**x)
    l1, dl, pl, el = (float(v) for v in FastSpeech2Loss(*flags).terms(after, before, d, p, e, ys, x["durations"], x["pitch"],
                                                                       x["energy"], x["text_lengths"], olens))
    _rel(got, {"l1_loss": l1, "duration_loss": dl, "pitch_loss": pl, "energy_loss": el, "loss": l1 + dl + pl + el})
    assert all(isinstance(v, float) and np.isfinite(v) and v > 0 for v in got.values())
    # the float32 tensors of the criterion itself are these numbers rounded
    t = FastSpeech2Loss(*flags)(after, before, d, p, e, ys, x["durations"], x["pitch"], x["energy"], x["text_lengths"], olens)
    assert [float(v) for v in t] == [float(np.float32(got[k])) for k in ("l1_loss", "duration_loss", "pitch_loss",
                                                                         "energy_loss")]


def test_fastspeech2_per_utterance_is_batch_independent_and_near_the_oracle():
    m, state, utts = _fs2()
    whole = m.evaluate_per_utterance(*_fs2_args(utts))
    outs = m.teacher_forced_batch(*_fs2_args(utts)[:4], return_before=True)
    d_engine = m.read_predictions()[0]
    for b, u in enumerate(utts):
        assert m.evaluate_per_utterance(*_fs2_args([u])) == [whole[b]]
        assert set(whole[b]) == {"l1_loss", "duration_loss", "pitch_loss", "energy_loss", "loss"}
        # an utterance alone through evaluate_batch: no padding, every mode the same numbers
        one = m.evaluate_batch(**_fs2_padded([u]))
        _rel(one, whole[b])
        _rel(m.evaluate_batch(**_fs2_padded([u]), use_masking=True), whole[b])
        ref = fref.forward(state, u["ids"], u["ds"], u["ps"], u["es"], fcases.case_cfg("t7"), dtype=torch.float64)
        y = u["mel"].astype(np.float64)
        l1_oracle = np.abs(ref["before"].numpy() - y).mean() + np.abs(ref["after"].numpy() - y).mean()
        room = (np.abs(_np(outs[b][0]) - ref["before"].numpy()).mean() + np.abs(_np(outs[b][1]) - ref["after"].numpy()).mean())
        print(f"FS2 utt {b}: l1 engine {whole[b]['l1_loss']:.9f} oracle {l1_oracle:.9f} room {room:.3e}")
        assert abs(whole[b]["l1_loss"] - l1_oracle) <= room
        want_d = ar.duration_predictor_loss(ref["d_outs"].numpy(), u["ds"])       # a squared norm of (d_outs - log targets)
        room_d = np.sqrt(((d_engine[b] - ref["d_outs"].numpy()) ** 2).mean())
        # ... whose targets the engine forms in float32: the sum's rounding and logf's ulp, at most 4u of the largest target
        assert abs(np.sqrt(whole[b]["duration_loss"]) - np.sqrt(want_d)) <= room_d + 4 * U * np.log(u["ds"].max() + 1.0)
    rev = m.evaluate_per_utterance(*_fs2_args(utts[::-1]))
    assert rev[::-1] == whole


# -------------------------------------------------------------------------------------------------------------- Tacotron2
def _taco():
    from parakeet_amd.tacotron2 import Tacotron2
    shape = {c[0]: c[1] for c in T2_CASES}["stop"]
    cfg = dict(syn.TACOTRON2_LJSPEECH, **shape)
    state = syn.tacotron2_state(cfg, seed=21, stop_bias=-8.0)
    m = Tacotron2(**cfg)
    m.set_state_dict(state)
    rng = np.random.default_rng(77)
    texts = [rng.integers(1, 37, size=T) for T in (5, 11, 3)]
    mels = [(0.5 * rng.standard_normal((L, 80))).astype(np.float32) for L in (7, 12, 2)]
    return m.eval(), cfg, state, texts, mels


OPTS = dict(use_stop_token_loss=True, use_guided_attention_loss=True, sigma=0.4)


def test_tacotron2_evaluate_batch_is_forward_then_the_criterion():
    from parakeet_amd.tacotron2 import Tacotron2Loss
    m, _, _, texts, mels = _taco()
    B, T, L = 3, max(len(t) for t in texts), max(len(y) for y in mels)
    x, y = np.zeros((B, T), np.int64), np.zeros((B, L, 80), np.float32)
    for b in range(B):
        x[b, :len(texts[b])], y[b, :len(mels[b])] = texts[b], mels[b]
    tl, ol = np.array([len(t) for t in texts]), np.array([len(v) for v in mels])
    got = m.evaluate_batch(x, tl, y, ol, seed=5, **OPTS)
    out = m.forward(x, tl, y, ol, seed=5)
    assert not np.any(_np(out["stop_logits"])[2, 2:])               # the engine's padded stop logits are zeros
    want = Tacotron2Loss(**OPTS).terms(out["mel_output"], out["mel_outputs_postnet"], y, out["alignments"], ol, tl,
                                       out["stop_logits"])
    _rel(got, {k: float(v) for k, v in want.items()})
    assert set(got) == {"loss", "mel_loss", "post_mel_loss", "guided_attn_loss", "stop_loss"}
    assert abs(got["loss"] - sum(v for k, v in got.items() if k != "loss")) <= 1e-12 * got["loss"]
    plain = m.evaluate_batch(x, tl, y, ol, seed=5, use_stop_token_loss=False)
    assert set(plain) == {"loss", "mel_loss", "post_mel_loss"} and plain["mel_loss"] == got["mel_loss"]


def test_tacotron2_per_utterance_is_batch_independent_and_near_the_oracle():
    m, cfg, state, texts, mels = _taco()
    seeds = [9, 21, 3]
    whole = m.evaluate_per_utterance(texts, mels, seeds=seeds, **OPTS)
    outs = m.teacher_forced_batch(texts, mels, seeds=seeds)
    for b in range(3):
        assert m.evaluate_per_utterance([texts[b]], [mels[b]], seeds=[seeds[b]], **OPTS) == [whole[b]]
        one = m.evaluate_batch(texts[b][None], [len(texts[b])], mels[b][None], [len(mels[b])], seed=seeds[b], **OPTS)
        _rel(one, whole[b])
        ref = tref.forward(state, texts[b], mels[b], cfg, seed=seeds[b], dtype=torch.float64)
        y = mels[b].astype(np.float64)
        for key, name in (("mel_output", "mel_loss"), ("mel_outputs_postnet", "post_mel_loss")):
            rms_oracle = np.sqrt(((ref[key].numpy() - y) ** 2).mean())
            room = np.sqrt(((_np(outs[b][key]) - ref[key].numpy()) ** 2).mean())
            print(f"Tacotron2 utt {b} {name}: rms engine {np.sqrt(whole[b][name]):.9f} oracle {rms_oracle:.9f} room {room:.3e}")
            assert abs(np.sqrt(whole[b][name]) - rms_oracle) <= room
    assert m.evaluate_per_utterance(texts[::-1], mels[::-1], seeds=seeds[::-1], **OPTS)[::-1] == whole


# --------------------------------------------------------------------------------------------------------- TransformerTTS
def _tts(**over):
    from parakeet_amd.transformer_tts import TransformerTTS
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, **dict(dict(elayers=1, dlayers=3, postnet_layers=2), **over))
    state = syn.transformer_tts_state(40, 80, cfg, seed=41, stop_bias=-6.0)
    m = TransformerTTS(idim=40, odim=80, **cfg)
    m.set_state_dict(state)
    rng = np.random.default_rng(11)
    texts = [syn.phoneme_ids(T, idim=40, seed=500 + T) for T in (7, 3, 5)]
    speech = [rng.standard_normal((L, 80)).astype(np.float32) for L in (23, 9, 14)]
    return m.eval(), cfg, state, texts, speech


def _tts_padded(texts, speech):
    B, T, L = len(texts), max(len(t) for t in texts), max(len(y) for y in speech)
    x, y = np.zeros((B, T), np.int64), np.zeros((B, L, 80), np.float32)
    for b in range(B):
        x[b, :len(texts[b])], y[b, :len(speech[b])] = texts[b], speech[b]
    return x, np.array([len(t) for t in texts]), y, np.array([len(v) for v in speech])


@pytest.mark.parametrize("r", [1, 2])
def test_transformer_tts_forward(r):
    m, cfg, _, texts, speech = _tts(reduction_factor=r)
    x, tl, y, ol = _tts_padded(texts, speech)
    seeds = [21, 22, 23]
    after, before, logits, ys, labels, olens, ilens, need = m.forward(x, tl, y, ol, seeds=seeds)
    w_labels, w_olens, w_ilens, n_ys = ar.transformer_tts_forward_targets(tl, ol, y.shape[1], r)
    assert np.array_equal(_np(labels), w_labels) and _np(labels).dtype == np.float32
    assert np.array_equal(_np(olens), w_olens) and np.array_equal(_np(ilens), w_ilens) and ys.shape[1] == n_ys
    assert tuple(after.shape) == tuple(before.shape) == (3, n_ys, 80) and tuple(logits.shape) == (3, n_ys)
    assert tuple(need["enc_dec_att_ws"].shape) == (3, cfg["dlayers"], cfg["aheads"], n_ys // r, x.shape[1] + 1)
    assert need["num_heads_applied_guided_attn"] == 2 and need["num_layers_applied_guided_attn"] == 2
    assert need["use_scaled_pos_enc"] is True and need["encoder_alpha"] is not None and need["decoder_alpha"] is not None
    worst = 0.0
    for b in range(3):
        n = (int(ol[b]) // r) * r
        assert np.array_equal(_np(before)[b, :n], m.debug_tap(1, b))              # bit for bit the engine's pre-postnet rows
        assert not np.any(_np(before)[b, n:]) and not np.any(_np(after)[b, n:]) and not np.any(_np(logits)[b, n:])
        lg, pr = _np(logits)[b, :n].astype(np.float64), _np(m.last_probs[b]).astype(np.float64)
        worst = max(worst, float((np.abs(1.0 / (1.0 + np.exp(-lg)) - pr) / pr).max()) / (2 * U))
        att = _np(need["enc_dec_att_ws"])[b, :, :, :n // r, :int(tl[b]) + 1]
        assert np.abs(att.sum(-1) - 1.0).max() < 1e-5
    print(f"SWEEP-RATIO tts stop probabilities against sigmoid(logits), r {r}: {worst:.4f}")
    assert worst <= 1.0
    # the teacher-forced outputs are what they were: forward() is teacher_forced_batch, padded
    outs = m.teacher_forced_batch(texts, speech, seeds)
    for b, (mel, _) in enumerate(outs):
        assert np.array_equal(_np(mel), _np(after)[b, :mel.shape[0]])
    # ... and the read call serves the teacher-forced pass only
    m.inference_batch([texts[1]], maxlenratio=1.0, seeds=[1])
    with pytest.raises(RuntimeError, match="pk_tts_teacher"):
        m._read_teacher()


def test_transformer_tts_evaluate_batch_is_forward_then_the_criteria():
    from parakeet_amd.transformer_tts import GuidedMultiHeadAttentionLoss, TransformerTTSLoss
    m, cfg, _, texts, speech = _tts()
    x, tl, y, ol = _tts_padded(texts, speech)
    seeds = [21, 22, 23]
    after, before, logits, ys, labels, olens, ilens, need = m.forward(x, tl, y, ol, seeds=seeds)
    att = need["enc_dec_att_ws"].as_subclass(torch.Tensor)[:, -2:, :2]          # last two layers, first two heads
    att = att.reshape(3, 4, att.shape[3], att.shape[4])
    for flags, pw, loss_type, sigma, lam in (((False, False), 5.0, "L1", 0.4, 1.0), ((True, False), 1.0, "L2", 0.2, 2.0),
                                             ((False, True), 5.0, "L1+L2", 0.4, 0.5)):
        got = m.evaluate_batch(x, tl, y, ol, seeds=seeds, use_masking=flags[0], use_weighted_masking=flags[1],
                               bce_pos_weight=pw, loss_type=loss_type, guided_attn_loss_sigma=sigma, guided_attn_loss_lambda=lam)
        l1, l2, bce = TransformerTTSLoss(*flags, bce_pos_weight=pw).terms(after, before, logits, ys, labels, olens)
        attn = GuidedMultiHeadAttentionLoss(sigma, lam).term(att, ilens, olens)
        want = {"bce_loss": bce, "l1_loss": l1, "l2_loss": l2, "enc_dec_attn_loss": attn,
                "encoder_alpha": need["encoder_alpha"], "decoder_alpha": need["decoder_alpha"],
                "loss": ar.transformer_tts_total(l1, l2, bce, loss_type) + attn}
        _rel(got, want)
        # the guided term is the restatement's on the same maps, within the derived bound of the sums
        ref = ar.guided_attention_loss_tts(_np(att), _np(ilens), _np(olens), sigma, lam)
        sums = ar.guided_sums(_np(att), _np(olens), _np(ilens), sigma)
        bound = lam * ar.guided_sums_bound(sigma, sums[:, 1], sums[:, 0], 0).sum() / float((4 * _np(olens) * _np(ilens)).sum())
        assert abs(got["enc_dec_attn_loss"] - ref) <= bound
    without = m.evaluate_batch(x, tl, y, ol, seeds=seeds, use_guided_attn_loss=False)
    assert "enc_dec_attn_loss" not in without and without["loss"] == without["l1_loss"] + without["bce_loss"]


def test_transformer_tts_per_utterance_is_batch_independent_and_near_the_oracle():
    m, cfg, state, texts, speech = _tts()
    seeds = [21, 22, 23]
    kw = dict(loss_type="L1+L2", bce_pos_weight=5.0)
    whole = m.evaluate_per_utterance(texts, speech, seeds=seeds, **kw)
    outs = m.teacher_forced_batch(texts, speech, seeds)
    before = [m.debug_tap(1, b) for b in range(3)]
    for b in range(3):
        assert m.evaluate_per_utterance([texts[b]], [speech[b]], seeds=[seeds[b]], **kw) == [whole[b]]
        one = m.evaluate_batch(texts[b][None], [len(texts[b])], speech[b][None], [len(speech[b])], seeds=[seeds[b]], **kw)
        _rel(one, whole[b])
        ref_after, _, parts = ttr.teacher_inference(state, texts[b], speech[b], cfg, seed=seeds[b])
        y = speech[b].astype(np.float64)
        ra, rb = ref_after.numpy(), parts["before"].numpy()
        l1_oracle = np.abs(ra - y).mean() + np.abs(rb - y).mean()
        room = np.abs(_np(outs[b][0]) - ra).mean() + np.abs(before[b] - rb).mean()
        print(f"TransformerTTS utt {b}: l1 engine {whole[b]['l1_loss']:.9f} oracle {l1_oracle:.9f} room {room:.3e}")
        assert abs(whole[b]["l1_loss"] - l1_oracle) <= room
        l2_oracle = ((ra - y) ** 2).mean() + ((rb - y) ** 2).mean()
        room2 = np.sqrt(((_np(outs[b][0]) - ra) ** 2).mean() + ((before[b] - rb) ** 2).mean())
        assert abs(np.sqrt(whole[b]["l2_loss"]) - np.sqrt(l2_oracle)) <= room2
    assert m.evaluate_per_utterance(texts[::-1], speech[::-1], seeds=seeds[::-1], **kw)[::-1] == whole


# --------------------------------------------------------------------------------------------------- examples' --score
def _example(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location("example_" + name, os.path.join(os.path.dirname(HERE), "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _printed(out, utt_id):
    line = [ln for ln in out.splitlines() if ln.startswith(utt_id + " ")][0]
    return {kv.split(": ")[0]: float(kv.split(": ")[1]) for kv in line[len(utt_id) + 1:].split(", ")}


def _same_to_six_decimals(printed, want):
    assert set(printed) == set(want)
    assert all(abs(printed[k] - want[k]) <= 0.5e-6 + 1e-12 for k in want), (printed, want)


def test_examples_score_prints_evaluate_per_utterance(tmp_path, capsys, monkeypatch):
    import json
    from parakeet_amd import checkpoint

    class Bound:
        def __init__(self, model):
            self.acoustic_model = model

        def bind(self):
            return self.acoustic_model

    # FastSpeech2
    m, _, utts = _fs2()
    lines = []
    for i, u in enumerate(utts):
        for k in ("ps", "es", "mel"):
            np.save(str(tmp_path / f"f{i}_{k}.npy"), u[k][:, None] if k != "mel" else u[k])
        lines.append(dict(utt_id=f"f{i}", text=[int(v) for v in u["ids"]], durations=[int(v) for v in u["ds"]],
                          pitch=f"f{i}_ps.npy", energy=f"f{i}_es.npy", feats=f"f{i}_mel.npy"))
    (tmp_path / "fs2.jsonl").write_text("".join(json.dumps(ln) + "\n" for ln in lines))
    monkeypatch.setattr(checkpoint, "load_fastspeech2", lambda *a, **k: (Bound(m), None))
    _example("fastspeech2_gta").main(["--fastspeech2-config", "-", "--fastspeech2-checkpoint", "-", "--fastspeech2-stat", "-",
                                      "--test-metadata", str(tmp_path / "fs2.jsonl"), "--output-dir", str(tmp_path / "o1"),
                                      "--score", "--batch-size", "2"])
    out = capsys.readouterr().out
    want = m.evaluate_per_utterance(*_fs2_args(utts))
    for i in range(3):
        _same_to_six_decimals(_printed(out, f"f{i}"), want[i])
    _same_to_six_decimals(_printed(out, "corpus mean"), {k: float(np.mean([w[k] for w in want])) for k in want[0]})
    # Tacotron2
    m, _, _, texts, mels = _taco()
    items = []
    for i in range(3):
        np.save(str(tmp_path / f"t{i}.npy"), mels[i])
        items.append(dict(utt_id=f"t{i}", text=texts[i], tones=None, mel=str(tmp_path / f"t{i}.npy"), global_condition=None))
    _example("tacotron2_gta").run(m, items, str(tmp_path / "o2"), seed=4, batch_size=2, score=True, guided_attention=True,
                                  sigma=0.4)
    out = capsys.readouterr().out
    want = m.evaluate_per_utterance(texts, mels, seeds=[4, 5, 6], **OPTS)
    for i in range(3):
        _same_to_six_decimals(_printed(out, f"t{i}"), want[i])
    # TransformerTTS
    m, _, _, texts, speech = _tts()
    lines = []
    for i in range(3):
        np.save(str(tmp_path / f"s{i}.npy"), speech[i])
        lines.append(dict(utt_id=f"s{i}", text=[int(v) for v in texts[i]], speech=f"s{i}.npy"))
    (tmp_path / "tts.jsonl").write_text("".join(json.dumps(ln) + "\n" for ln in lines))
    monkeypatch.setattr(checkpoint, "load_transformer_tts", lambda *a, **k: (Bound(m), None))
    _example("transformer_tts_gta").main(["--transformer-tts-config", "-", "--transformer-tts-checkpoint", "-",
                                          "--transformer-tts-stat", "-", "--test-metadata", str(tmp_path / "tts.jsonl"),
                                          "--output-dir", str(tmp_path / "o3"), "--seed", "21", "--score", "--loss-type", "L2"])
    out = capsys.readouterr().out
    want = m.evaluate_per_utterance(texts, speech, seeds=[21, 22, 23], loss_type="L2")
    for i in range(3):
        _same_to_six_decimals(_printed(out, f"s{i}"), want[i])
    assert os.path.exists(str(tmp_path / "o3" / "s2_gta.npy")) and os.path.exists(str(tmp_path / "o1" / "f0_gta.npy"))
