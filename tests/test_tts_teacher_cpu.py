"""TransformerTTS teacher forcing without a GPU: the fp64 restatement (tests/tts_teacher_ref.py) against the reference's own
source (tests/golden/tts_teacher.npz, tools/make_golden_tts_teacher.py), the dropout steps of the golden generator's hook,
and the argument / metadata parsing of examples/transformer_tts_gta.py."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

from parakeet_amd import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ar_cases import TTS_CASES  # noqa: E402
import tts_teacher_ref as ttr  # noqa: E402

GOLD = os.path.join(HERE, "golden")
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("case", [c[0] for c in TTS_CASES])
def test_restatement_matches_reference_source(case):
    name, over, idim, T, seed, skw, kw = [c for c in TTS_CASES if c[0] == case][0]
    g = np.load(os.path.join(GOLD, "tts_teacher.npz"))
    cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, **over)
    state = syn.transformer_tts_state(idim, 80, cfg, seed=seed, **skw)
    spemb = g[f"{name}_spemb"] if f"{name}_spemb" in g else None
    y = g[f"{name}_speech"]
    r = cfg.get("reduction_factor", 1)
    if r > 1:
        assert y.shape[0] % r != 0                                                   # a length that is not a multiple of r
    mel, att, parts = ttr.teacher_inference(state, g[f"{name}_ids"], y, cfg, seed=seed, spembs=spemb, dtype=torch.float64)
    assert mel.shape == g[f"{name}_mel"].shape == ((y.shape[0] // r) * r, 80)
    assert att.shape == g[f"{name}_att"].shape == (cfg["dlayers"], cfg["aheads"], y.shape[0] // r, T + 1)
    assert np.abs(mel.numpy() - g[f"{name}_mel"]).max() < 2e-5
    assert np.abs(att.numpy() - g[f"{name}_att"]).max() < 2e-6
    # the generator's hook saw one prenet call per layer, each on all L // r rows: step = row count = L // r
    rows = list(g[f"{name}_drop_rows"])
    assert rows == [y.shape[0] // r] * (cfg["dprenet_layers"])
    assert parts["drop_steps"] == rows


def test_dropout_element_index_is_the_ar_call_at_step_l_in():
    """The teacher pass's prenet mask is the AR decode's mask at step s = L_in (include/pk_synth.h dropout stream)."""
    from oracle import transformer_tts_ref as tt
    drop = tt.stream_dropout(3, 2, 16)
    s = 7
    keep = drop(s, 1, s, 16)
    from oracle import philox_ref
    idx = ((s * (s - 1) // 2 + np.arange(s, dtype=np.uint64)[:, None]) * 2 + 1) * 16 + np.arange(16, dtype=np.uint64)[None]
    assert np.array_equal(keep, philox_ref.dropout_keep(idx.astype(np.uint64), 0.5, 3))


def _example():
    spec = importlib.util.spec_from_file_location("transformer_tts_gta", os.path.join(ROOT, "examples", "transformer_tts_gta.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_arguments_and_metadata(tmp_path):
    ex = _example()
    a = ex.parse_args(["--transformer-tts-config", "c.yaml", "--transformer-tts-checkpoint", "s.pdz", "--transformer-tts-stat",
                       "st.npy", "--phones-dict", "p.txt", "--test-metadata", "m.jsonl", "--output-dir", "out"])
    assert (a.test_metadata, a.output_dir, a.seed, a.batch_size, a.save_attention) == ("m.jsonl", "out", 0, 32, False)
    a = ex.parse_args(["--transformer-tts-config", "c", "--transformer-tts-checkpoint", "s", "--transformer-tts-stat", "t",
                       "--test-metadata", "m", "--output-dir", "o", "--save-attention", "--batch-size", "4", "--seed", "3"])
    assert (a.save_attention, a.batch_size, a.seed, a.phones_dict) == (True, 4, 3, "phone_id_map.txt")
    with pytest.raises(SystemExit):
        ex.parse_args(["--transformer-tts-config", "c"])                             # --test-metadata etc. required
    (tmp_path / "sub").mkdir()
    meta = tmp_path / "metadata.jsonl"
    meta.write_text(json.dumps({"utt_id": "LJ001-0001", "text": [3, 4, 5], "speech": "sub/a.npy", "speech_lengths": 9}) + "\n\n" +
                    json.dumps({"utt_id": "LJ001-0002", "text": [7], "speech": "/abs/b.npy"}) + "\n")
    items = ex.read_metadata(str(meta))
    assert [i[0] for i in items] == ["LJ001-0001", "LJ001-0002"]
    assert items[0][1].dtype == np.int64 and list(items[0][1]) == [3, 4, 5]
    assert items[0][2] == os.path.join(str(tmp_path), "sub/a.npy") and items[1][2] == "/abs/b.npy"
