"""GE2E speaker encoder on the device (csrc/spk.hip through the C ABI) against the fp64 restatement tests/ge2e_ref.py.

Error bars: the embeddings are unit vectors; the contract is max-abs < 1e-4 against the fp64 oracle in both maths.
The regression bars (MAX_ERR) are 10x the error measured on an MI355X (noted per case)."""
import os
import sys

import numpy as np
import pytest
import torch

from parakeet_amd import ge2e_audio, synthetic as syn
from parakeet_amd.lstm_speaker_encoder import LSTMSpeakerEncoder

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ge2e_ref  # noqa: E402

pytestmark = pytest.mark.gpu

RELEASED = syn.GE2E_RELEASED
SECOND = dict(n_mels=80, num_layers=2, hidden_size=128, output_size=64)
CONTRACT = 1e-4
# 10x the max-abs error measured on an MI355X (released f16x3 1.09e-7, f32 1.33e-7; second f16x3 1.70e-7, f32 2.39e-7)
MAX_ERR = {"released-f16x3": 1.1e-6, "released-f32": 1.4e-6, "second-f16x3": 1.7e-6, "second-f32": 2.4e-6}
MEL_MAX_REL = 1.2e-5   # 10x the power-mel relative error measured on an MI355X (1.17e-6)


def _model(cfg, seed, math="f16x3", state=None):
    m = LSTMSpeakerEncoder(**cfg)
    m.set_state_dict(state if state is not None else syn.ge2e_state(cfg, seed=seed))
    m.eval()
    m.set_math(math)
    return m


def _partials(P, T, n_mels, seed):
    """Power-mel-like inputs: magnitudes spread over decades, as the front end produces."""
    rng = np.random.default_rng(seed)
    return (np.exp(rng.normal(-2.0, 2.0, size=(P, T, n_mels)))).astype(np.float32)


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("math", ["f16x3", "f32"])
@pytest.mark.parametrize("shape", ["released", "second"])
def test_embed_vs_oracle(shape, math):
    cfg, T, P = (RELEASED, 160, 37) if shape == "released" else (SECOND, 37, 45)   # P not a multiple of 32: a tile tail
    st = syn.ge2e_state(cfg, seed=11)
    m = _model(cfg, 11, math, st)
    x = _partials(P, T, cfg["n_mels"], seed=1)
    got = m.embed_sequences(x).cpu().numpy()
    ref = ge2e_ref.embed_sequences(st, x, cfg["num_layers"]).numpy()
    err = _err(got, ref)
    print(f"GE2E {shape} {math}: max-abs {err:.3e}")
    assert err < min(CONTRACT, MAX_ERR[f"{shape}-{math}"]), f"{shape} {math}: max-abs {err:.3e}"
    utt = m.embed_utterance(x).cpu().numpy()
    ref_u = ge2e_ref.embed_sequences(st, x, cfg["num_layers"], reduce=True).numpy()
    assert utt.shape == (cfg["output_size"],)
    assert _err(utt, ref_u) < CONTRACT


@pytest.mark.parametrize("math", ["f16x3", "f32"])
def test_initial_states(math):
    cfg = SECOND
    st = syn.ge2e_state(cfg, seed=12)
    m = _model(cfg, 12, math, st)
    P, T, L, H = 9, 21, cfg["num_layers"], cfg["hidden_size"]
    x = _partials(P, T, cfg["n_mels"], seed=2)
    rng = np.random.default_rng(3)
    h0 = (rng.standard_normal((L, P, H)) * 0.8).astype(np.float32)
    c0 = (rng.standard_normal((L, P, H)) * 2.0).astype(np.float32)
    got = m.embed_sequences(x, initial_states=(h0, c0)).cpu().numpy()
    ref = ge2e_ref.embed_sequences(st, x, L, initial_states=(h0, c0)).numpy()
    assert _err(got, ref) < CONTRACT
    # initial states matter: the zero-state result differs
    assert _err(m.embed_sequences(x).cpu().numpy(), got) > 1e-3


@pytest.mark.parametrize("math", ["f16x3", "f32"])
def test_batch_invariance(math):
    """A ragged embed_utterances of 1, 3 and 8 partials equals per-utterance calls bit for bit."""
    m = _model(RELEASED, 13, math)
    batches = [_partials(n, 160, 40, seed=20 + n) for n in (1, 3, 8)]
    together = m.embed_utterances(batches).cpu().numpy()
    for u, b in enumerate(batches):
        alone = m.embed_utterance(b).cpu().numpy()
        assert np.array_equal(together[u], alone), f"utterance {u} ({len(b)} partials) differs"
    seqs = m.embed_sequences(np.concatenate(batches)).cpu().numpy()
    assert np.array_equal(seqs[4:12], m.embed_sequences(batches[2]).cpu().numpy())


def test_large_batch_spot_check():
    """4 100 partials in one call: three spot-checked against the oracle, and bit-equal to a call of their own."""
    st = syn.ge2e_state(RELEASED, seed=14)
    m = _model(RELEASED, 14, "f16x3", st)
    P = 4100
    x = _partials(P, 160, 40, seed=4)
    got = m.embed_sequences(x).cpu().numpy()
    assert np.isfinite(got).all()
    pick = [0, 2049, P - 1]
    ref = ge2e_ref.embed_sequences(st, x[pick], 3).numpy()
    assert _err(got[pick], ref) < CONTRACT
    assert np.array_equal(got[pick], m.embed_sequences(x[pick]).cpu().numpy())


def test_hidden_512():
    cfg = dict(n_mels=40, num_layers=1, hidden_size=512, output_size=256)
    st = syn.ge2e_state(cfg, seed=15)
    for math in ("f16x3", "f32"):
        m = _model(cfg, 15, math, st)
        x = _partials(33, 12, 40, seed=5)
        assert _err(m.embed_sequences(x).cpu().numpy(), ge2e_ref.embed_sequences(st, x, 1).numpy()) < CONTRACT


def test_single_step():
    st = syn.ge2e_state(RELEASED, seed=16)
    m = _model(RELEASED, 16, "f16x3", st)
    x = _partials(5, 1, 40, seed=6)
    assert _err(m.embed_sequences(x).cpu().numpy(), ge2e_ref.embed_sequences(st, x, 3).numpy()) < CONTRACT


def test_all_zero_relu():
    st = syn.ge2e_state(RELEASED, seed=17)
    st["linear.bias"] = np.full(256, -100.0, dtype=np.float32)
    m = _model(RELEASED, 17, "f16x3", st)
    x = _partials(4, 20, 40, seed=7)
    e = m.embed_sequences(x).cpu().numpy()
    u = m.embed_utterance(x).cpu().numpy()
    assert np.isfinite(e).all() and np.isfinite(u).all()
    assert not e.any() and not u.any()


@pytest.mark.parametrize("H", [100, 544, 0])
def test_unsupported_hidden_size(H):
    with pytest.raises(ValueError):
        LSTMSpeakerEncoder(40, 3, H, 256)


def test_forward_is_training():
    m = _model(RELEASED, 18)
    with pytest.raises(NotImplementedError):
        m.forward(_partials(2, 4, 40, 0), 1)


def test_wav_to_partials():
    """Front end on the engine (pad, power mel of the whole wav once, slice) against the fp64 restatement."""
    pre = ge2e_audio.ge2e_preprocessor(overlap=0.75)
    clips = [ge2e_ref.synthetic_clip(s, seed=30 + i) for i, s in enumerate((0.7, 4.0, 5.3))]
    wavs = [pre.preprocess_wav(c) for c in clips]
    got = pre.extract_mel_partials_batch(wavs)
    assert [g.shape[0] for g in got] == [1, 8, 11]
    for w, g in zip(wavs, got):
        _, sl = ge2e_audio.compute_partial_slices(len(w), 160, 160, 0.75, 0.75)
        pad = np.pad(w, (0, max(0, 160 * (sl[-1].stop) - len(w))))
        ref = ge2e_ref.mel_partials(pad, [s.start for s in sl]).numpy()
        g = g.cpu().numpy()
        rel = np.abs(g - ref).max() / np.abs(ref).max()
        print(f"power mel relative error {rel:.3e}")
        assert rel < MEL_MAX_REL, f"power mel relative error {rel:.3e}"
    one = pre.extract_mel_partials(wavs[1]).cpu().numpy()
    assert np.array_equal(one, got[1].cpu().numpy())


def test_encoder_to_tacotron2_condition():
    """The embedding handed to Tacotron2(d_global_condition=256) as a device tensor gives the mel it gives as numpy."""
    from parakeet_amd.tacotron2 import Tacotron2
    enc = _model(RELEASED, 19)
    emb = enc.embed_utterance(_partials(4, 160, 40, seed=8))
    cfg = dict(syn.TACOTRON2_LJSPEECH, d_global_condition=256)
    tst = syn.tacotron2_state(cfg, seed=21)
    kw = {k: v for k, v in cfg.items()}
    taco = Tacotron2(**kw)
    taco.set_state_dict(tst)
    taco.eval()
    ids = np.array([[3, 5, 7, 9, 11, 2, 4]], dtype=np.int64)
    a = taco.infer(ids, max_decoder_steps=30, global_condition=emb[None], seed=1)["mel_outputs_postnet"].cpu().numpy()
    b = taco.infer(ids, max_decoder_steps=30, global_condition=emb.cpu().numpy()[None], seed=1)["mel_outputs_postnet"]
    assert np.array_equal(a, b.cpu().numpy())
    assert np.isfinite(a).all()


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ge2e.npz")   # tools/make_golden_ge2e.py


@pytest.mark.parametrize("math", ["f16x3", "f32"])
@pytest.mark.parametrize("shape", ["released", "second"])
def test_embed_vs_reference_golden(shape, math):
    """The engine against the reference's own embed_sequences / embed_utterance (fp32, stand-in Paddle)."""
    g = np.load(GOLD)
    cfg = RELEASED if shape == "released" else SECOND
    m = _model(cfg, int(g[f"{shape}_seed"]), math)
    x = g[f"{shape}_x"]
    assert _err(m.embed_sequences(x).cpu().numpy(), g[f"{shape}_seqs"]) < CONTRACT
    assert _err(m.embed_utterance(x).cpu().numpy(), g[f"{shape}_utt"]) < CONTRACT


def test_front_end_vs_reference_golden():
    """wav -> partials on the engine against the reference's extract_mel_partials (overlap 0.75)."""
    g = np.load(GOLD)
    pre = ge2e_audio.ge2e_preprocessor(overlap=0.75)
    got = pre.extract_mel_partials_batch([pre.preprocess_wav(g[f"clip{i}"]) for i in range(2)])
    for i in range(2):
        want = g[f"partials{i}"]
        have = got[i].cpu().numpy()
        assert have.shape == want.shape
        assert np.abs(have - want).max() / np.abs(want).max() < MEL_MAX_REL


def test_load_ge2e_round_trip(tmp_path):
    """A step-N.pdparams written as paddle.save writes a state dict, loaded through checkpoint.load_ge2e (with and
    without the suffix), embeds like the model given the same state directly."""
    import importlib.util
    from parakeet_amd import checkpoint
    spec = importlib.util.spec_from_file_location("mkfix", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "make_paddle_fixture.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    st = syn.ge2e_state(RELEASED, seed=22)
    mk.paddle_save({k: mk.VarBase(f"param_{i}", v) for i, (k, v) in enumerate(st.items())},
                   str(tmp_path / "step-100.pdparams"))
    x = _partials(3, 160, 40, seed=9)
    want = _model(RELEASED, 22, state=st).embed_utterance(x).cpu().numpy()
    for path in (tmp_path / "step-100", tmp_path / "step-100.pdparams"):
        enc = checkpoint.load_ge2e(path)
        assert np.array_equal(enc.embed_utterance(x).cpu().numpy(), want)


def _fixture_writer():
    import importlib.util
    spec = importlib.util.spec_from_file_location("mkfix", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "make_paddle_fixture.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return lambda st, path: mk.paddle_save({k: mk.VarBase(f"param_{i}", v) for i, (k, v) in enumerate(st.items())},
                                           str(path))


def _run_example(name, args):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", name)] + [str(a) for a in args],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_example_ge2e_inference(tmp_path):
    """examples/ge2e_inference.py on a small corpus: one .npy per wav at the same relative path, equal to
    embed_utterance of the wav at overlap 0.75 (inference.py:81)."""
    from parakeet_amd.audio import write_wav
    save = _fixture_writer()
    st = syn.ge2e_state(RELEASED, seed=23)
    save(st, tmp_path / "step-5.pdparams")
    corpus = tmp_path / "wavs"
    rels = ["a/s1.wav", "a/s2.wav", "b/c/s3.wav"]
    for i, rel in enumerate(rels):
        (corpus / rel).parent.mkdir(parents=True, exist_ok=True)
        write_wav(str(corpus / rel), ge2e_ref.synthetic_clip(1.0 + 1.5 * i, seed=40 + i), 16000)
    _run_example("ge2e_inference.py", ["--input", corpus, "--output", tmp_path / "emb", "--checkpoint_path",
                                       tmp_path / "step-5", "--batch", 2])
    pre = ge2e_audio.ge2e_preprocessor(overlap=0.75)
    m = _model(RELEASED, 23, state=st)
    for rel in rels:
        got = np.load(tmp_path / "emb" / rel.replace(".wav", ".npy"))
        want = m.embed_utterance(pre.extract_mel_partials(pre.preprocess_wav(str(corpus / rel)))).cpu().numpy()
        assert got.shape == (256,)
        assert np.array_equal(got, want)


def test_example_voice_cloning(tmp_path):
    """examples/voice_cloning.py end to end with seeded weights of the notebook's shapes: one finite WAV per line."""
    from parakeet_amd.audio import write_wav
    save = _fixture_writer()
    save(syn.ge2e_state(RELEASED, seed=24), tmp_path / "ge2e.pdparams")
    tcfg = dict(syn.TACOTRON2_LJSPEECH, vocab_size=68, n_tones=10, d_global_condition=256, use_stop_token=False)
    save(syn.tacotron2_state(tcfg, seed=25), tmp_path / "taco.pdparams")
    save(syn.waveflow_state(dict(syn.WAVEFLOW_LJSPEECH, channels=128), seed=26), tmp_path / "wf.pdparams")
    write_wav(str(tmp_path / "ref.wav"), ge2e_ref.synthetic_clip(3.0, seed=50), 16000)
    (tmp_path / "text.txt").write_text("u1 | 3 5 7 9 11 2 | 1 2 3 4 1 2\nu2 | 4 6 8 | 2 2 5\n")
    _run_example("voice_cloning.py", ["--ref_audio", tmp_path / "ref.wav", "--ge2e_checkpoint", tmp_path / "ge2e",
                                      "--tacotron2_checkpoint", tmp_path / "taco.pdparams", "--waveflow_checkpoint",
                                      tmp_path / "wf.pdparams", "--text", tmp_path / "text.txt", "--output_dir",
                                      tmp_path / "out", "--max_decoder_steps", 20])
    for utt in ("u1", "u2"):
        assert (tmp_path / "out" / f"{utt}.wav").stat().st_size > 44
