"""TransformerTTS.inference(..., use_teacher_forcing=True) on the HIP engine (csrc/tts_teacher.hip, pk_tts_teacher): the
reference's own source (tests/golden/tts_teacher.npz, tools/make_golden_tts_teacher.py), the fp64 restatement
(tests/tts_teacher_ref.py), ragged batches, self-consistency with the AR decode, seeds, refusals and the GTA example."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import transformer_tts_ref as tt
from parakeet_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ar_cases import TTS_CASES  # noqa: E402
import tts_teacher_ref as ttr  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)


def _model(cfg, idim, state, math=None):
    from parakeet_amd.transformer_tts import TransformerTTS
    m = TransformerTTS(idim=idim, odim=80, **cfg)
    m.set_state_dict(state)
    m.eval()
    if math:
        m.set_math(math)
    return m


def _close(a, b, l1=1e-4, mx=2e-3):   # the tolerances of tests/test_tts_gpu.py's AR goldens
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.abs(a - b).mean() < l1 and np.abs(a - b).max() < mx


def _case(name):
    return [c for c in TTS_CASES if c[0] == name][0]


@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("case", [c[0] for c in TTS_CASES])
def test_teacher_matches_reference_source(case, math):
    name, over, idim, T, seed, skw, kw = _case(case)
    g = np.load(os.path.join(GOLD, "tts_teacher.npz"))
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, **over)
    state = syn.transformer_tts_state(idim, 80, cfg, seed=seed, **skw)
    m = _model(cfg, idim, state, math)
    spemb = g[f"{name}_spemb"] if f"{name}_spemb" in g else None
    mel, probs, att = m.inference(g[f"{name}_ids"], speech=g[f"{name}_speech"], spembs=spemb, use_teacher_forcing=True,
                                  seed=seed)
    assert probs is None
    assert _close(mel.cpu().numpy(), g[f"{name}_mel"]), np.abs(mel.cpu().numpy() - g[f"{name}_mel"]).max()
    assert _close(att.cpu().numpy(), g[f"{name}_att"])
    _, _, parts = ttr.teacher_inference(state, g[f"{name}_ids"], g[f"{name}_speech"], cfg, seed=seed, spembs=spemb)
    assert _close(m.debug_tap(1, 0), parts["before"].numpy())                    # pre-postnet frames


@pytest.mark.parametrize("math", ["f32", "f16x3"])
def test_recipe_sizes_against_fp64_restatement(math):
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH)
    state = syn.transformer_tts_state(60, 80, cfg, seed=31, stop_bias=-6.0)
    texts = [syn.phoneme_ids(T, idim=60, seed=400 + T) for T in (120, 96)]
    rng = np.random.default_rng(5)
    speech = [rng.standard_normal((L, 80)).astype(np.float32) for L in (640, 611)]
    m = _model(cfg, 60, state, math)
    outs = m.teacher_forced_batch(texts, speech, seeds=[3, 4])
    for b, (t, y, (mel, att)) in enumerate(zip(texts, speech, outs)):
        ref, ratt, parts = ttr.teacher_inference(state, t, y, cfg, seed=3 + b)
        d_mel = np.abs(mel.cpu().numpy() - ref.numpy())
        d_att = np.abs(att.cpu().numpy() - ratt.numpy())
        d_hs = np.abs(m.debug_tap(0, b) - parts["hs"].numpy())
        d_zs = np.abs(m.debug_tap(2, b) - parts["zs"].numpy())
        d_bf = np.abs(m.debug_tap(1, b) - parts["before"].numpy())
        print(f"[{math}] utt {b}: mel mean {d_mel.mean():.2e} max {d_mel.max():.2e}; att max {d_att.max():.2e}; "
              f"hs max {d_hs.max():.2e}; zs max {d_zs.max():.2e}; before max {d_bf.max():.2e}")
        assert d_mel.mean() <= 1e-5
        assert d_att.max() < 1e-4 and d_bf.max() < 2e-4 and d_zs.max() < 2e-4 and d_hs.max() < 1e-4
        assert np.abs(att.cpu().numpy().sum(-1) - 1.0).max() < 1e-5


@pytest.mark.parametrize("math", ["f32", "f16x3"])
def test_ragged_batch_is_bitwise_the_single_calls(math):
    rng = np.random.default_rng(11)
    for over, idim, skw, extra in [
        (dict(elayers=1, dlayers=2, postnet_layers=2), 40, dict(stop_bias=-6.0), {}),
        (dict(elayers=1, dlayers=2, postnet_layers=2, reduction_factor=2), 40, dict(stop_bias=-6.0), {}),
        (dict(elayers=1, dlayers=1, postnet_layers=0, reduction_factor=3), 40, dict(stop_bias=-6.0), {}),
        (dict(elayers=1, dlayers=1, postnet_layers=0, use_gst=True, spk_embed_dim=32, spk_embed_integration_type="add"), 40,
         dict(stop_bias=-6.0), dict(spk=32)),
    ]:
        cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, **over)
        state = syn.transformer_tts_state(idim, 80, cfg, seed=41, **skw)
        m = _model(cfg, idim, state, math)
        Ts, Ls = (7, 3, 12, 5, 9, 1), (23, 70, 41, 8, 100, 5)
        texts = [syn.phoneme_ids(T, idim=idim, seed=500 + T) for T in Ts]
        speech = [rng.standard_normal((L, 80)).astype(np.float32) for L in Ls]
        seeds = [21, 22, 23, 24, 25, 26]
        sp = rng.standard_normal((6, extra["spk"])).astype(np.float32) if "spk" in extra else None
        outs = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in m.teacher_forced_batch(texts, speech, seeds, spembs=sp)]
        taps = [m.debug_tap(1, b) for b in range(6)]
        for b in range(6):
            one = m.teacher_forced_batch([texts[b]], [speech[b]], [seeds[b]], spembs=None if sp is None else sp[b:b + 1])[0]
            assert np.array_equal(one[0].cpu().numpy(), outs[b][0]), (over, b)
            assert np.array_equal(one[1].cpu().numpy(), outs[b][1]), (over, b)
            assert np.array_equal(m.debug_tap(1, 0), taps[b])


@pytest.mark.parametrize("over", [
    dict(),
    dict(reduction_factor=2),
    dict(reduction_factor=3),
    dict(decoder_normalize_before=False),
    dict(decoder_concat_after=True),
    dict(decoder_normalize_before=False, decoder_concat_after=True),
    dict(spk_embed_dim=48, spk_embed_integration_type="add"),
    dict(spk_embed_dim=48, spk_embed_integration_type="concat"),
])
def test_self_consistency_with_ar_decode(over):
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, elayers=1, dlayers=2, postnet_layers=2, **over)
    state = syn.transformer_tts_state(40, 80, cfg, seed=61, stop_bias=-6.0)
    m = _model(cfg, 40, state, "f32")
    m.set_dropout(False)
    texts = [syn.phoneme_ids(T, idim=40, seed=600 + T) for T in (6, 9, 4)]
    sp = None
    if cfg.get("spk_embed_dim"):
        sp = np.random.default_rng(3).standard_normal((3, 48)).astype(np.float32)
    ar = m.inference_batch(texts, maxlenratio=2.0, spembs=sp)
    ar = [(a.cpu().numpy(), c.cpu().numpy()) for a, _, c in ar]
    before = [m.debug_tap(1, b) for b in range(3)]
    tf = m.teacher_forced_batch(texts, before, spembs=sp)
    for b in range(3):
        mel, att = tf[b][0].cpu().numpy(), tf[b][1].cpu().numpy()
        for x, y in ((m.debug_tap(1, b), before[b]), (att, ar[b][1]), (mel, ar[b][0])):
            d = np.abs(np.asarray(x, np.float64) - y)
            assert x.shape == y.shape and d.mean() <= 1e-5 and d.max() <= 1e-4, (over, b, d.mean(), d.max())


def test_seeds_and_dropout_switch():
    name, over, idim, T, seed, skw, kw = _case("lj")
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, **over)
    state = syn.transformer_tts_state(idim, 80, cfg, seed=seed, **skw)
    m = _model(cfg, idim, state)
    ids = syn.phoneme_ids(T, idim=idim, seed=1)
    y = np.random.default_rng(2).standard_normal((30, 80)).astype(np.float32)
    a = m.inference(ids, speech=y, use_teacher_forcing=True, seed=1)[0].cpu().numpy()
    assert np.array_equal(a, m.inference(ids, speech=y, use_teacher_forcing=True, seed=1)[0].cpu().numpy())
    b = m.inference(ids, speech=y, use_teacher_forcing=True, seed=2)[0].cpu().numpy()
    assert np.abs(a - b).max() > 1e-3
    m.set_dropout(False)
    c = m.inference(ids, speech=y, use_teacher_forcing=True)[0].cpu().numpy()
    ref = ttr.teacher_inference(state, ids, y, cfg, dropout=False)[0].numpy()
    assert _close(c, ref)
    assert not _close(a, ref)


def test_refusals_and_state():
    name, over, idim, T, seed, skw, kw = _case("lj")
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, **over)
    m = _model(cfg, idim, syn.transformer_tts_state(idim, 80, cfg, seed=seed, **skw))
    g = np.load(os.path.join(GOLD, "transformer_tts.npz"))
    ids = g[f"{name}_ids"]
    ref_mel = g[f"{name}_mel"]
    assert _close(m.inference(ids, seed=seed, **kw)[0].cpu().numpy(), ref_mel)
    y = np.random.default_rng(2).standard_normal((30, 80)).astype(np.float32)
    with pytest.raises(AssertionError):
        m.inference(ids, use_teacher_forcing=True)                               # no speech (:569)
    with pytest.raises(ValueError):
        m.inference(ids, speech=y[:, :40], use_teacher_forcing=True)             # wrong width
    m.inference(ids, speech=y, use_teacher_forcing=True, seed=3)                 # a teacher call between two AR calls
    assert _close(m.inference(ids, seed=seed, **kw)[0].cpu().numpy(), ref_mel)
    # reduction factor 2: L < r refused, L = r accepted
    c2 = dict(syn.TRANSFORMER_TTS_LJSPEECH, elayers=1, dlayers=1, postnet_layers=0, reduction_factor=2)
    m2 = _model(c2, 40, syn.transformer_tts_state(40, 80, c2, seed=5, stop_bias=-6.0))
    with pytest.raises(ValueError):
        m2.inference(ids, speech=y[:1], use_teacher_forcing=True)
    assert m2.inference(ids, speech=y[:2], use_teacher_forcing=True)[0].shape == (2, 80)
    assert m2.inference(ids, speech=y[:5], use_teacher_forcing=True)[0].shape == (4, 80)
    # a speaker model without spembs
    c3 = dict(syn.TRANSFORMER_TTS_LJSPEECH, elayers=1, dlayers=1, postnet_layers=0, spk_embed_dim=16)
    m3 = _model(c3, 40, syn.transformer_tts_state(40, 80, c3, seed=6, stop_bias=-6.0))
    with pytest.raises(ValueError):
        m3.inference(ids, speech=y, use_teacher_forcing=True)
    assert m3.inference(ids, speech=y, spembs=np.ones(16, np.float32), use_teacher_forcing=True)[0].shape == (30, 80)
    # the token envelope: what the AR decode's step kernel holds (64-wide heads: 14260 keys incl. <eos>)
    c4 = dict(syn.TRANSFORMER_TTS_LJSPEECH, elayers=1, dlayers=1, postnet_layers=0, adim=64, aheads=1, eunits=64, dunits=64,
              dprenet_units=64)
    m4 = _model(c4, 40, syn.transformer_tts_state(40, 80, c4, seed=7, stop_bias=-6.0))
    edge = syn.phoneme_ids(14259, idim=40, seed=8)
    mel, _, att = m4.inference(edge, speech=y[:4], use_teacher_forcing=True)
    assert mel.shape == (4, 80) and att.shape == (1, 1, 4, 14260) and np.isfinite(mel.cpu().numpy()).all()
    with pytest.raises(NotImplementedError):
        m4.inference(np.concatenate([edge, edge[:1]]), speech=y[:4], use_teacher_forcing=True)
    assert m4.inference(ids, speech=y[:4], use_teacher_forcing=True)[0].shape == (4, 80)   # the handle stays usable


def test_gta_example(tmp_path):
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, elayers=1, dlayers=1, postnet_layers=2)
    state = syn.transformer_tts_state(40, 80, cfg, seed=71, stop_bias=-6.0)
    import pickle
    import yaml
    ckpt = tmp_path / "snapshot.pdz"
    with open(ckpt, "wb") as f:
        pickle.dump({"main_params": {k: ("t", v) for k, v in state.items()}}, f, protocol=2)
    conf = tmp_path / "default.yaml"
    conf.write_text(yaml.safe_dump({"fs": 22050, "n_mels": 80, "model": dict(cfg)}))
    stats = tmp_path / "speech_stats.npy"
    np.save(str(stats), np.stack([np.full(80, -4.0, np.float32), np.full(80, 0.5, np.float32)]))
    phones = tmp_path / "phone_id_map.txt"
    phones.write_text("".join(f"P{i} {i}\n" for i in range(40)))
    rng = np.random.default_rng(4)
    meta = tmp_path / "metadata.jsonl"
    items = []
    for i, (T, L) in enumerate([(5, 17), (8, 30), (3, 9)]):
        y = rng.standard_normal((L, 80)).astype(np.float32)
        np.save(str(tmp_path / f"u{i}_speech.npy"), y)
        items.append(dict(utt_id=f"u{i}", text=[int(v) for v in syn.phoneme_ids(T, idim=40, seed=i)],
                          speech=str(tmp_path / f"u{i}_speech.npy")))
    meta.write_text("".join(json.dumps(it) + "\n" for it in items))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "transformer_tts_gta.py"),
                        "--transformer-tts-config", str(conf), "--transformer-tts-checkpoint", str(ckpt),
                        "--transformer-tts-stat", str(stats), "--phones-dict", str(phones), "--test-metadata", str(meta),
                        "--output-dir", str(out), "--save-attention", "--batch-size", "2", "--seed", "9"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = _model(cfg, 40, state)
    for i, it in enumerate(items):
        gta = np.load(str(out / f"u{i}_gta.npy"))
        att = np.load(str(out / f"u{i}_att.npy"))
        y = np.load(it["speech"])
        mel, _, a = m.inference(np.array(it["text"]), speech=y, use_teacher_forcing=True, seed=9 + i)
        assert gta.shape == tuple(mel.shape) and np.abs(gta - mel.cpu().numpy()).max() < 1e-5
        assert att.shape == tuple(a.shape)
