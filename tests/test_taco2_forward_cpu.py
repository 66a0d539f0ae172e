"""Tacotron2 with teacher forcing, CPU side: the fp32 restatement (tests/taco2_forward_ref.py) against the golden vectors
the reference's own ``Tacotron2.forward`` produced (tools/make_golden_taco_forward.py -> golden/tacotron2_forward.npz),
and the new export of the C boundary."""
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import taco2_forward_cases as cases  # noqa: E402
import taco2_forward_ref as fref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "tacotron2_forward.npz")
TOL = 2e-5      # the oracle <-> golden bar of tests/test_golden_cpu.py (max-abs, fp32 restatement vs fp32 reference source)


def test_golden_file_holds_every_case():
    g = np.load(GOLD)
    assert str(g["cases"]).split(",") == list(cases.CASES)
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "tacotron2.npz"))
    for name in cases.CASES:        # the stored inputs are the ones the case table regenerates
        u = cases.case_inputs(name)
        for k in ("ids", "tones", "global_condition", "mels", "output_lens"):
            if u[k] is None:
                assert f"{name}_{k}" not in g.files
            else:
                assert np.array_equal(g[f"{name}_{k}"], u[k]), (name, k)
        assert list(g[f"{name}_seeds"]) == u["seeds"]
        assert (f"{name}_stop_logits" in g.files) == bool(cases.case_cfg(name)["use_stop_token"])


def _restate(name, b, dtype=torch.float32, **kw):
    u = cases.case_inputs(name)
    return fref.forward(cases.case_state(name), u["ids"][b], u["mels"][b], cases.case_cfg(name),
                        tones=None if u["tones"] is None else u["tones"][b], seed=u["seeds"][b], dtype=dtype,
                        global_condition=None if u["global_condition"] is None else u["global_condition"][b],
                        output_len=None if u["output_lens"] is None else int(u["output_lens"][b]), **kw)


def test_restatement_matches_reference_source():
    g = np.load(GOLD)
    for name in cases.CASES:
        u = cases.case_inputs(name)
        for b in range(u["ids"].shape[0]):
            out = _restate(name, b)
            for k in cases.KEYS:
                if f"{name}_{k}" not in g.files:
                    assert k not in out
                    continue
                got, want = out[k].numpy(), g[f"{name}_{k}"][b]
                assert got.shape == want.shape, (name, k)
                assert np.abs(got - want).max() < TOL, (name, k, np.abs(got - want).max())
            assert np.abs(out["alignments"].numpy().sum(-1) - 1.0).max() < 1e-5


def test_output_mask_of_the_batch_case():
    """``output_lens`` zeroes mel rows only (:765-769); alignments and stop logits of the padded frames stay."""
    g = np.load(GOLD)
    L = int(g["batch2_output_lens"][1])
    assert L < g["batch2_mels"].shape[1]
    for k in ("mel_output", "mel_outputs_postnet"):
        assert not np.any(g[f"batch2_{k}"][1, L:]) and np.all(np.any(g[f"batch2_{k}"][1, :L] != 0, axis=-1))
        assert np.all(np.any(g[f"batch2_{k}"][0] != 0, axis=-1))
    assert np.all(g["batch2_alignments"][1, L:].sum(-1) > 0.99) and np.all(g["batch2_stop_logits"][1, L:] != 0)


def test_teacher_is_live_and_causal_in_the_restatement():
    name = "stop"
    u = cases.case_inputs(name)
    cfg, state = cases.case_cfg(name), cases.case_state(name)
    a = fref.forward(state, u["ids"][0], u["mels"][0], cfg, seed=3)
    k = 4
    mel = u["mels"][0].copy()
    mel[k] += 1.0
    b = fref.forward(state, u["ids"][0], mel, cfg, seed=3)
    for key in ("mel_output", "alignments", "stop_logits"):
        assert np.array_equal(a[key].numpy()[:k + 1], b[key].numpy()[:k + 1]), key     # frame k is the query of step k + 1
    assert np.abs(a["mel_output"].numpy()[k + 1] - b["mel_output"].numpy()[k + 1]).max() > 1e-4
    # the last teacher frame is never a query (:455-456)
    mel = u["mels"][0].copy()
    mel[-1] += 1.0
    c = fref.forward(state, u["ids"][0], mel, cfg, seed=3)
    assert np.array_equal(a["mel_output"].numpy(), c["mel_output"].numpy())


def test_restatement_agrees_with_free_running_oracle_on_its_own_output():
    """Teacher-forcing the oracle's ``infer`` output reproduces it: the two restatements share every step."""
    from oracle import tacotron2_ref as t2
    name = "stop"
    u = cases.case_inputs(name)
    cfg, state = cases.case_cfg(name), cases.case_state(name)
    free = t2.infer(state, u["ids"][0], cfg, max_decoder_steps=7, seed=5, dtype=torch.float64)
    tf = fref.forward(state, u["ids"][0], free["mel_output"].numpy(), cfg, seed=5, dtype=torch.float64)
    for k in cases.KEYS:
        assert np.abs(free[k].numpy() - tf[k].numpy()).max() < 1e-12, k


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "pk_synth.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, set(re.findall(r"\b(pk_[a-z0-9_]+)\s*\(", text))


def test_new_export_in_header_binding_and_library():
    import __graft_entry__ as ge
    ge.build()
    from parakeet_amd import _capi
    lib = _capi.lib()
    bound = _capi._declare(lib)
    text, declared = _declared_symbols()
    s = "pk_taco_teacher"
    assert s in declared, f"include/pk_synth.h does not declare {s}"
    assert s in bound, f"_capi does not bind {s}"
    assert hasattr(lib, s), f"libpk_synth.so does not export {s}"
    args = re.search(r"\b%s\s*\(([^)]*)\)" % s, text).group(1)
    assert len(bound[s][1]) == len(args.split(","))
