"""The autoregressive step kernels and the per-step dispatch of TransformerTTS (csrc/tts.hip) and Tacotron2 (csrc/taco2.hip) over
the shapes they admit, through ``TransformerTTS.inference_batch`` / ``Tacotron2.infer_batch`` and the debug taps, against the
float64 oracles under the bars of tests/ar_step_cases.py (4 x the float32 oracle's own error, from the references alone).
``SWEEP-RATIO ar_step <case> <quantity> <error / bar>`` before every assertion.

Per call: every compared quantity of every utterance under its bar (``x:mean``: the mean per frame, at every step), every
utterance's length equal to the oracle's, attention and alignment rows summing to one, and the profile showing the kernels the case
is meant to run.  The profile gives every instantiation of a step kernel one name (tts_attn_self, tts_attn_src, taco_lsa_ctx ...), so
WHICH template or how many threads ran is not observable here; the boundary table of the case file and the dispatch claims of
tests/test_ar_step_cpu.py stand for that.
"""
import functools

import numpy as np
import pytest

import ar_step_cases as ac

pytestmark = pytest.mark.gpu

TTS_PARAMS = [(c, m) for c, v in ac.TTS_CALLS.items() for m in v["maths"]]
T2_PARAMS = [(c, m) for c, v in ac.T2_CALLS.items() for m in v["maths"]]


def _profiled(fn):
    """fn() with the profile on -> (its result, names of the kernels that ran)."""
    from parakeet_amd.runtime import Context
    ctx = Context.get()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        out = fn()
        names = {k for k, (n, _) in ctx.prof_dump().items() if n > 0}
    finally:
        ctx.prof_enable(False)
    return out, names


def _report(tag, ref, runs, quantities):
    r = ac.ratios(ref, runs, quantities)
    for q, v in r.items():
        print(f"SWEEP-RATIO ar_step {tag} {q} {v:.4f}   (bar {ref['bar'][q]:.3e})")
    for q, v in r.items():
        assert v <= 1.0, f"{tag} {q}: error {v:.3f} x the bar {ref['bar'][q]:.3e}"
    return r


# ---- TransformerTTS ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _tts_model_of(model, seed):
    from parakeet_amd.transformer_tts import TransformerTTS
    m = TransformerTTS(idim=ac.TTS_IDIM, odim=ac.ODIM, **ac.tts_config(model))
    m.set_state_dict(ac.tts_state(model, seed))
    m.eval()
    return m


def _tts_model(call):
    """The engine model of a call (kept for the call's second math): the weights the call's references were computed with."""
    return _tts_model_of(ac.TTS_CALLS[call]["model"], ac.SEEDS.get(call, {}).get("model"))


def _tts_run(model, call, math, n=None):
    """One ``inference_batch`` of the call's first ``n`` utterances -> (one dict per utterance, kernel names)."""
    c = ac.TTS_CALLS[call]
    texts = ac.tts_texts(call)[:n]
    model.set_math(math)
    outs, names = _profiled(lambda: model.inference_batch(texts, maxlenratio=c["ratio"], seeds=ac.drop_seeds(len(texts))))
    runs = [dict(hs=model.debug_tap(0, b), before=model.debug_tap(1, b), zs=model.debug_tap(2, b), probs=o[1].cpu().numpy(),
                 att=o[2].cpu().numpy(), mel=o[0].cpu().numpy()) for b, o in enumerate(outs)]
    return runs, names


@pytest.mark.parametrize("call,math", TTS_PARAMS, ids=[f"{c}-{m}" for c, m in TTS_PARAMS])
def test_tts_step_sweep(call, math):
    c, ref = ac.TTS_CALLS[call], ac.tts_reference(call)
    runs, names = _tts_run(_tts_model(call), call, math)
    assert [r["before"].shape[0] for r in runs] == ref["lengths"]
    _report(f"{call}-{math}", ref, runs, ac.TTS_QUANTITIES)
    for r in runs:
        assert np.array_equal(r["mel"], r["before"])                                 # no postnet
        assert np.abs(r["att"].sum(-1) - 1.0).max() < 1e-5
    assert "tts_attn_self" in names, names
    M = ac.TTS_MODELS[c["model"]]
    if ac.src_q_fused(M["adim"] // M["aheads"], max(c["keys"]), M["adim"]):      # group 2 at K <= 256 (and the tiny texts of 3 and 4)
        assert "tts_attn_src_q" in names and "tts_attn_src" not in names and "tts_row_src_q" not in names, names
    else:
        assert "tts_attn_src" in names and "tts_row_src_q" in names and "tts_attn_src_q" not in names, names
    if c["group"] == 4:
        assert "tts_stop" in names and "tts_row_feat_out" in names and "tts_row_feat_out_stop" not in names, names
    else:
        assert "tts_row_feat_out_stop" in names and "tts_stop" not in names, names


def test_tts_33_utterances_against_the_first_32():
    """The B = 32 call of the first 32 utterances (one row block, the stop head on the feat_out row GEMM) against the B = 33 call
    (two row blocks, k_tts_stop with the LayerNorm): the same bits for every utterance -- encoder and decoder rows, spectrogram,
    attention weights, and the stop probabilities too, although another kernel computes them."""
    call = "tts-b33"
    model, ref = _tts_model(call), ac.tts_reference(call)
    r33, _ = _tts_run(model, call, "f16x3")
    r32, names = _tts_run(model, call, "f16x3", n=32)
    assert "tts_row_feat_out_stop" in names and "tts_stop" not in names, names
    _report(f"{call}-B32", dict(ref, utts=ref["utts"][:32]), r32, ac.TTS_QUANTITIES)
    for b in range(32):
        assert r32[b]["before"].shape == r33[b]["before"].shape, b
        for k in ("hs", "zs", "before", "att", "probs"):
            assert np.array_equal(r32[b][k], r33[b][k]), f"utterance {b}: {k} differs between B = 32 and B = 33"


# ---- Tacotron2 -----------------------------------------------------------------------------------------------------------------
T2_KEYS = ("mel_output", "mel_outputs_postnet", "alignments", "stop_logits")


@functools.lru_cache(maxsize=2)
def _t2_model_of(model, seed):
    from parakeet_amd.tacotron2 import Tacotron2
    m = Tacotron2(**ac.t2_config(model))
    m.set_state_dict(ac.t2_state(model, seed))
    m.eval()
    return m


def _t2_model(call):
    return _t2_model_of(ac.T2_CALLS[call]["model"], ac.SEEDS.get(call, {}).get("model"))


def _t2_run(model, call, math, order=None):
    """One ``infer_batch`` of the call's utterances ``order`` (default: all, table order) -> (dict per utterance in that order, names)."""
    c = ac.T2_CALLS[call]
    order = list(range(len(c["T"]))) if order is None else list(order)
    texts, gc, seeds = ac.t2_texts(call), ac.t2_global_condition(call), ac.drop_seeds(len(c["T"]))
    model.set_math(math)
    outs, names = _profiled(lambda: model.infer_batch([texts[b] for b in order], max_decoder_steps=c["steps"],
                                                      seeds=[seeds[b] for b in order],
                                                      global_condition=None if gc is None else gc[order]))
    runs = []
    for i, o in enumerate(outs):
        r = {k: o[k].cpu().numpy() for k in T2_KEYS if k in o}
        r["enc"] = model.debug_tap(0, i)
        runs.append(r)
    return runs, names


@pytest.mark.parametrize("call,math", T2_PARAMS, ids=[f"{c}-{m}" for c, m in T2_PARAMS])
def test_t2_step_sweep(call, math):
    c, ref = ac.T2_CALLS[call], ac.t2_reference(call)
    model = _t2_model(call)
    runs, names = _t2_run(model, call, math)
    assert [r["mel_output"].shape[0] for r in runs] == ref["lengths"]
    _report(f"{call}-{math}", ref, runs, ac.T2_QUANTITIES)
    for r in runs:
        assert np.abs(r["alignments"].sum(-1) - 1.0).max() < 1e-5
        assert ("stop_logits" in r) == (c["group"] != 9)
    assert {"taco_lstm_seq", "taco_lsa_energy", "taco_lsa_ctx"} <= names, names
    if ac.fused_prenet(ac.t2_config(c["model"])["d_prenet"]):
        assert "taco_prenet" in names and "taco_row_prenet" not in names, names
    else:
        assert "taco_row_prenet" in names and "taco_prenet" not in names, names
    if c["group"] in (8, 9):                                              # B > 32 with a stop token; the no-stop rule
        assert "taco_stop" in names and "taco_row_proj" in names and "taco_row_proj_stop" not in names, names
    else:
        assert "taco_row_proj_stop" in names and "taco_stop" not in names, names
    if c["group"] == 5:                                                   # the reversed batch: the same bits per utterance
        n = len(c["T"])
        rev, _ = _t2_run(model, call, math, order=range(n - 1, -1, -1))
        for b, r in enumerate(rev[::-1]):
            for k in r:
                assert np.array_equal(r[k], runs[b][k]), f"{call}: utterance of {c['T'][b]} tokens differs between the batch orders ({k})"


def test_t2_33_utterances_against_the_first_32():
    """As the TransformerTTS test: B = 32 (the stop token on the projection's row GEMM) against B = 33 (taco_row_proj +
    k_taco_stop): the same bits for every utterance, the stop logits of the other kernel included."""
    call = "t2-b33"
    model, ref = _t2_model(call), ac.t2_reference(call)
    r33, _ = _t2_run(model, call, "f16x3")
    r32, names = _t2_run(model, call, "f16x3", order=range(32))
    assert "taco_row_proj_stop" in names and "taco_stop" not in names, names
    _report(f"{call}-B32", dict(ref, utts=ref["utts"][:32]), r32, ac.T2_QUANTITIES)
    for b in range(32):
        assert r32[b]["mel_output"].shape == r33[b]["mel_output"].shape, b
        for k in ("enc", "mel_output", "mel_outputs_postnet", "alignments", "stop_logits"):
            assert np.array_equal(r32[b][k], r33[b][k]), f"utterance {b}: {k} differs between B = 32 and B = 33"


def test_t2_teacher_forced_row_prenet():
    """``forward()`` of the d_prenet = 48 model: k_taco_teacher_prenet with w1 == NULL builds the shifted query rows only, the loop
    keeps the row-GEMM prenet with dropout in its epilogue.  Against tests/taco2_forward_ref.py in float64."""
    import torch
    call = ac.TEACHER_CALL
    c, ref = ac.T2_CALLS[call], ac.t2_teacher_reference(call)
    model = _t2_model(call)
    model.set_math("f16x3")
    texts, mels = ac.t2_texts(call), ac.teacher_mels(call)
    Tmax = max(c["T"])
    padded = np.zeros((len(texts), Tmax), dtype=np.int64)
    for b, t in enumerate(texts):
        padded[b, :len(t)] = t
    out, names = _profiled(lambda: model.forward(padded, np.array(c["T"]), torch.from_numpy(mels), seed=0))
    assert "taco_teacher_prenet" in names and "taco_row_prenet" in names and "taco_prenet_rows" not in names, names
    runs = []
    for b, T in enumerate(c["T"]):
        r = {k: out[k].cpu().numpy()[b] for k in T2_KEYS}
        assert not r["alignments"][:, T:].any()
        r["alignments"] = r["alignments"][:, :T]
        r["enc"] = model.debug_tap(0, b)
        runs.append(r)
    _report(f"{call}-teacher", ref, runs, ac.T2_QUANTITIES)
