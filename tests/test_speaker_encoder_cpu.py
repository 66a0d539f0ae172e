"""GE2E speaker encoder: the oracle and the front end on the CPU (no device)."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

from parakeet_amd import ge2e_audio, synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ge2e_ref  # noqa: E402


def test_restatement_matches_torch_lstm():
    """The fp64 restatement against torch.nn.LSTM with the same weights, initial states included."""
    cfg = dict(n_mels=24, num_layers=2, hidden_size=32, output_size=32)
    st = syn.ge2e_state(cfg, seed=5)
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 11, 24)).astype(np.float32)
    h0 = rng.standard_normal((2, 3, 32)) * 0.5
    c0 = rng.standard_normal((2, 3, 32)) * 0.5
    lstm = torch.nn.LSTM(24, 32, 2, batch_first=True).double()
    with torch.no_grad():
        for name, p in lstm.named_parameters():
            p.copy_(torch.from_numpy(st["lstm." + name].astype(np.float64)))
        for init in (None, (h0, c0)):
            _, (h, _) = lstm(torch.from_numpy(x).double(),
                             None if init is None else tuple(torch.from_numpy(s) for s in init))
            mine = ge2e_ref.lstm_last_hidden(st, x, 2, init)
            assert torch.allclose(mine, h[-1], atol=1e-12)


def test_normalize_zero_vector():
    e = ge2e_ref.normalize(torch.zeros(2, 4, dtype=torch.float64), 1)
    assert torch.equal(e, torch.zeros(2, 4, dtype=torch.float64))


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ge2e.npz")   # tools/make_golden_ge2e.py
SHAPES = {"released": syn.GE2E_RELEASED, "second": dict(n_mels=80, num_layers=2, hidden_size=128, output_size=64)}


def _gold():
    return np.load(GOLD)


def test_compute_partial_slices_vs_reference():
    """The reference's own compute_partial_slices (audio_processor.py:110-170) on edge cases: 0.75 overlap, coverage
    drops, a clip shorter than one partial, overlap 0 and 0.9."""
    g = _gold()
    o = 0
    for (n, ov, cov), cnt in zip(g["slice_cases"], g["slice_counts"]):
        wav_s, mel_s = ge2e_audio.compute_partial_slices(int(n), 160, 160, float(cov), float(ov))
        assert [s.start for s in mel_s] == list(g["slice_starts"][o:o + cnt]), (n, ov, cov)
        assert all(s.stop - s.start == 160 for s in mel_s)
        assert [(w.start, w.stop) for w in wav_s] == [(m.start * 160, m.stop * 160) for m in mel_s]
        o += cnt
    assert o == len(g["slice_starts"])


def test_front_end_vs_reference():
    """preprocess_wav's volume step and the pad -> mel -> slice path of extract_mel_partials (audio_processor.py:201-246)
    against the reference run at inference.py's overlap 0.75; the mel is the restatement on both sides."""
    g = _gold()
    pre = ge2e_audio.ge2e_preprocessor(overlap=0.75)
    for i in range(2):
        wav = ge2e_audio.normalize_volume(g[f"clip{i}"].astype(np.float32), -30, increase_only=True)
        np.testing.assert_allclose(wav, g[f"wav{i}"], rtol=1e-6, atol=0)
        padded, starts = pre._padded(g[f"wav{i}"])
        got = ge2e_ref.mel_partials(padded, starts).numpy()
        want = g[f"partials{i}"]
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert g["partials1"].shape[0] == 8   # a 4 s clip at overlap 0.75


@pytest.mark.parametrize("shape", ["released", "second"])
def test_restatement_vs_reference(shape):
    """The fp64 restatement (head included: relu(linear), normalize, mean, normalize) against the reference's
    LSTMSpeakerEncoder.embed_sequences / embed_utterance run in fp32 on the same weights."""
    g = _gold()
    cfg = SHAPES[shape]
    st = syn.ge2e_state(cfg, seed=int(g[f"{shape}_seed"]))
    x = g[f"{shape}_x"]
    seqs = ge2e_ref.embed_sequences(st, x, cfg["num_layers"]).numpy()
    utt = ge2e_ref.embed_sequences(st, x, cfg["num_layers"], reduce=True).numpy()
    assert np.abs(seqs - g[f"{shape}_seqs"]).max() < 2e-6
    assert np.abs(utt - g[f"{shape}_utt"]).max() < 2e-6


def test_partial_counts_of_a_4s_clip():
    """The trap of examples/ge2e/inference.py:81: overlap 0.75 (its corpus tool) gives 8 partials, 0.5 gives 4."""
    assert len(ge2e_audio.compute_partial_slices(64000, 160, 160, 0.75, 0.75)[1]) == 8
    assert len(ge2e_audio.compute_partial_slices(64000, 160, 160, 0.75, 0.5)[1]) == 4


def test_normalize_volume():
    wav = np.full(100, 0.001, dtype=np.float64)
    out = ge2e_audio.normalize_volume(wav, -30, increase_only=True)
    assert np.isclose(10 * np.log10(np.mean(out ** 2)), -30)
    loud = np.full(100, 0.5)
    assert ge2e_audio.normalize_volume(loud, -30, increase_only=True) is loud
    assert np.isclose(10 * np.log10(np.mean(ge2e_audio.normalize_volume(loud, -30) ** 2)), -30)
    with pytest.raises(ValueError):
        ge2e_audio.normalize_volume(wav, -30, increase_only=True, decrease_only=True)


def test_state_aliases():
    st = syn.ge2e_state(seed=1)
    for k in range(3):
        for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            assert st[f"lstm.{p}_l{k}"] is st[f"lstm.{k}.cell.{p}"]
    assert st["lstm.weight_ih_l0"].shape == (1024, 40) and st["linear.weight"].shape == (256, 256)


def test_pdparams_round_trip():
    """A step-N.pdparams written the way paddle.save writes a state dict reads back through the existing reader."""
    import importlib.util
    from parakeet_amd import checkpoint
    spec = importlib.util.spec_from_file_location("mkfix", os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools", "make_paddle_fixture.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    st = syn.ge2e_state(dict(n_mels=40, num_layers=1, hidden_size=32, output_size=32), seed=3)
    params = {k: mk.VarBase(f"param_{i}", v) for i, (k, v) in enumerate(st.items())}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "step-10.pdparams")
        mk.paddle_save(params, path)
        back = checkpoint.load_params(path)
    assert set(back) == set(st)
    for k, v in st.items():
        np.testing.assert_array_equal(np.asarray(back[k]), v)
