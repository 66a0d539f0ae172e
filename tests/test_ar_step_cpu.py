"""The inputs and the bars of the autoregressive step sweep (tests/ar_step_cases.py) are worth something: no GPU.

Dispatch claims.  The shapes of every case fall on the side of each boundary of ``attn_step()`` / ``taco_run()`` that the case
table claims, by the one-line restatements in the case file: a moved boundary shows up here, not as a sweep that quietly tests
something else.

Bars.  Every bar is 4 x max(float32 oracle's own error, one float32 ulp of the peak) and none is looser than the fixed bar the
existing tests hold the same quantity to (decoding feeds back: a badly conditioned input would otherwise buy itself a wide bar).

Input conditions, from the float64 oracles alone: weight on the last 16-key group at the last step (TransformerTTS groups 1 - 3),
on the last position and beyond position 256 (Tacotron2 groups 5 and 9), stop decisions and alignment maxima that are not marginal
(groups 4, 8, 9), and the mix of endings groups 4 and 8 are about.

Planted defects.  Each of the ways a step kernel could be subtly wrong, planted in the oracle through its hooks, moves some
compared quantity of its target call above that call's bar.

``SWEEP-RATIO`` lines give error / bar; ``AR-STEP-E32`` lines the table of DESIGN.md.
"""
import numpy as np
import pytest
import torch

import ar_step_cases as ac

TTS_BY_GROUP = {g: [c for c, v in ac.TTS_CALLS.items() if v["group"] == g] for g in (1, 2, 3, 4)}
T2_BY_GROUP = {g: [c for c, v in ac.T2_CALLS.items() if v["group"] == g] for g in (5, 6, 7, 8, 9)}


def _dk(call):
    m = ac.TTS_MODELS[ac.TTS_CALLS[call]["model"]]
    return m["adim"] // m["aheads"], m["adim"]


# ---- dispatch claims -----------------------------------------------------------------------------------------------------------
def test_dispatch_head_sizes_take_the_general_kernel():
    seen = []
    for call in TTS_BY_GROUP[1]:
        dk, adim = _dk(call)
        seen.append((dk, 256 // (dk // 4)))
        assert dk // 4 > 16                                             # more float4 columns than one 16-lane pass
        assert not ac.src_q_fused(dk, max(ac.TTS_CALLS[call]["keys"]), adim)
        assert {ac.attn_step_choice(dk, n) for n in range(1, 258)} == {"general"}
        assert ac.tts_reference(call)["lengths"][0] == 70               # self keys walk through 16, 64 and 65
    assert seen == [(96, 10), (128, 8), (192, 5), (192, 5)]             # (dk, value groups G); 5 x 48 = 240: 16 idle threads


SRC_CLAIMS = {128: (True, "step64<8,q>"), 129: (True, "step64<16,q>"), 256: (True, "step64<16,q>"), 257: (False, "step64<24>"),
              384: (False, "step64<24>"), 385: (False, "step64<32>"), 512: (False, "step64<32>"), 513: (False, "step64<40>"),
              640: (False, "step64<40>"), 641: (False, "general")}


def test_dispatch_source_key_boundaries():
    assert tuple(SRC_CLAIMS) == ac.SRC_KEYS
    for call in TTS_BY_GROUP[2]:
        dk, adim = _dk(call)
        K = max(ac.TTS_CALLS[call]["keys"])
        fused = ac.src_q_fused(dk, K, adim)
        assert dk == 64 and (fused, ac.attn_step_choice(dk, K, fused)) == SRC_CLAIMS[K], call
        assert ac.tts_reference(call)["lengths"] == [3, 1, 1]


def test_dispatch_self_key_boundaries():
    (call,) = TTS_BY_GROUP[3]
    dk, _ = _dk(call)
    L = ac.tts_reference(call)["lengths"]
    assert L == [649, 433]
    walk = [ac.attn_step_choice(dk, s) for s in range(1, L[0] + 1)]
    for s, (at, after) in {128: ("step64<8>", "step64<16>"), 256: ("step64<16>", "step64<24>"), 384: ("step64<24>", "step64<32>"),
                           512: ("step64<32>", "step64<40>"), 640: ("step64<40>", "general")}.items():
        assert (walk[s - 1], walk[s]) == (at, after), s
    assert walk[-1] == "general"


def test_dispatch_tacotron2_widths():
    assert len(ac.TTS_CALLS["tts-b33"]["keys"]) == len(ac.T2_CALLS["t2-b33"]["T"]) == 33        # > PK_RG_ROWS = 32: a second row block
    E = [ac.t2_config(m)["d_encoder"] for m in ("enc32", "enc96", "enc544")]
    assert [ac.lstm_threads(e // 2) for e in E] == [64, 192, 1024] and 4 * (E[2] // 2) == 1088
    assert [e + 16 for e in E] == [48, 112, 560] and -(-560 // 256) == 3 and 560 - 512 == 48
    pre = {m: ac.t2_config(m)["d_prenet"] for m in ("pre16", "pre48", "pre48p25", "pre512")}
    assert pre == dict(pre16=16, pre48=48, pre48p25=48, pre512=512)
    assert [ac.fused_prenet(p) for p in pre.values()] == [True, False, False, True]
    assert ac.fused_prenet(64) and ac.fused_prenet(256)                 # what the older tests run
    for m, want in (("lsa-min", (16, 1, 1)), ("lsa-max", (256, 64, 63)), ("lsa-base", (64, 8, 7))):
        c = ac.t2_config(m)
        assert (c["d_attention"], c["attention_filters"], c["attention_kernel_size"]) == want
    assert {t % 16 for t in ac.LSA_T} >= {0, 1, 15} and max(ac.LSA_T) > 256 and min(ac.LSA_T) == 1


# ---- bars ----------------------------------------------------------------------------------------------------------------------
def _check_bars(tag, ref, quantities):
    for q in quantities:
        if q not in ref["bar"]:
            continue
        e32, peak, bar = ref["e32"][q], ref["peak"][q], ref["bar"][q]
        print(f"AR-STEP-E32 {tag} {q} e32 {e32:.3e} peak {peak:.3f} bar {bar:.3e} fixed {ac.FIXED_BAR[q]:.0e}")
        assert bar == 4.0 * max(e32, ac.ulp32(peak)) and np.isfinite(bar) and bar > 0.0
    for q in quantities:
        if q in ref["bar"]:
            assert ref["bar"][q] <= ac.FIXED_BAR[q], f"{tag} {q}: derived bar {ref['bar'][q]:.3e} looser than {ac.FIXED_BAR[q]:.0e}"


@pytest.mark.parametrize("call", list(ac.TTS_CALLS))
def test_tts_reference_and_bar(call):
    ref = ac.tts_reference(call)
    print(f"AR-STEP-CPU {call} group {ac.TTS_CALLS[call]['group']} references {ref['seconds']:.1f} s, lengths {ref['lengths']}")
    for r, k in zip(ref["utts"], ac.TTS_CALLS[call]["keys"]):
        assert r["hs"].shape[0] == r["att"].shape[-1] == k
        np.testing.assert_allclose(r["att"].sum(-1), 1.0, rtol=0, atol=1e-12)
    _check_bars(call, ref, ac.TTS_QUANTITIES)


@pytest.mark.parametrize("call", list(ac.T2_CALLS))
def test_t2_reference_and_bar(call):
    ref = ac.t2_reference(call)
    print(f"AR-STEP-CPU {call} group {ac.T2_CALLS[call]['group']} references {ref['seconds']:.1f} s, lengths {ref['lengths']}")
    for r, T in zip(ref["utts"], ac.T2_CALLS[call]["T"]):
        assert r["enc"].shape[0] == r["alignments"].shape[1] == T
    _check_bars(call, ref, ac.T2_QUANTITIES)
    if call == ac.TEACHER_CALL:
        _check_bars(call + "-teacher", ac.t2_teacher_reference(), ac.T2_QUANTITIES)


# ---- input conditions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", TTS_BY_GROUP[1] + TTS_BY_GROUP[2] + TTS_BY_GROUP[3])
def test_tts_tail_keys_carry_weight(call):
    src, own = ac.tts_tail_weights(ac.tts_reference(call)["utts"][0])
    print(f"AR-STEP-INPUT {call} weight on the last 16-key group at the last step: source {src:.3f}, self {own:.3f}")
    assert src >= ac.TAIL_WEIGHT_MIN and own >= ac.TAIL_WEIGHT_MIN


@pytest.mark.parametrize("call", T2_BY_GROUP[5] + T2_BY_GROUP[9])
def test_t2_tail_positions_carry_weight(call):
    ref = ac.t2_reference(call)
    last = {}
    for T, r in zip(ac.T2_CALLS[call]["T"], ref["utts"]):
        w_last, w_far = ac.t2_tail_weights(r)
        print(f"AR-STEP-INPUT {call} T {T}: largest weight on the last position {w_last:.3f}, beyond position 256 {w_far}")
        last[T] = w_last
        if T >= 257:
            assert w_far >= ac.TAIL_WEIGHT_MIN, (T, w_far)
    assert max(w for T, w in last.items() if T >= 2) >= ac.TAIL_WEIGHT_MIN, last


def _endings(lengths, caps, stopped):
    """The mix groups 4 and 8 are about: several end steps, two at the cap, utterance 32 through the stop token at a step of its own."""
    assert len(lengths) == 33 and len(set(lengths)) >= 3, lengths
    assert sum(L == c for L, c in zip(lengths, caps)) >= 2, (lengths, caps)
    assert sum(stopped) >= 3 and stopped[32] and lengths[32] < caps[32] and lengths.count(lengths[32]) == 1, lengths


def test_tts_stop_decisions_are_not_marginal():
    ref = ac.tts_reference("tts-b33")
    c = ac.TTS_CALLS["tts-b33"]
    margin = min(ac.stop_margin_tts(r) for r in ref["utts"])
    print(f"AR-STEP-INPUT tts-b33 smallest |p - 0.5| {margin:.3f}, lengths {ref['lengths']}")
    assert margin >= ac.STOP_PROB_MARGIN
    _endings(ref["lengths"], [int(k * c["ratio"]) for k in c["keys"]], [r["probs"][-1] >= 0.5 for r in ref["utts"]])


def test_t2_stop_decisions_are_not_marginal():
    ref = ac.t2_reference("t2-b33")
    margin = min(float(np.abs(r["stop_logits"]).min()) for r in ref["utts"])
    print(f"AR-STEP-INPUT t2-b33 smallest |logit| {margin:.3f}, lengths {ref['lengths']}")
    assert margin >= ac.STOP_LOGIT_MARGIN
    _endings(ref["lengths"], [ac.T2_CALLS["t2-b33"]["steps"]] * 33, [r["stop_logits"][-1] > 0 for r in ref["utts"]])


def test_t2_content_exhausted_rule_is_not_marginal():
    ref = ac.t2_reference("nostop")
    T = ac.T2_CALLS["nostop"]["T"]
    assert T[0] == 1 and ref["lengths"][0] == 22                     # argmax on the last position from step 0: ends at step 0 + 21
    for t, r in zip(T[1:], ref["utts"][1:]):
        top = np.sort(r["alignments"], axis=-1)
        gap = float((top[:, -1] - top[:, -2]).min())
        print(f"AR-STEP-INPUT nostop T {t}: smallest gap of the top two alignment entries {gap:.2e}, length {r['alignments'].shape[0]}")
        assert gap >= ac.TOP2_MARGIN


# ---- planted defects -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", sorted(ac.TTS_DEFECTS))
def test_tts_planted_defect_is_rejected(defect):
    what, hook, call, n = ac.TTS_DEFECTS[defect]
    ref = ac.tts_reference(call)
    runs = [ac.tts_oracle(call, b, torch.float64, attn_hook=hook) if b == n else None for b in range(len(ref["utts"]))]
    r = ac.ratios(ref, runs, ("zs", "before", "probs"))
    print(f"SWEEP-RATIO ar_step defect tts-{defect} {call} " + " ".join(f"{q} {v:.1f}" for q, v in r.items()))
    assert max(r.values()) > 1.0, f"{what}: under the bars {r}"


def test_tts_hook_that_changes_nothing_reproduces_the_reference():
    ref = ac.tts_reference("src-129")
    run = ac.tts_oracle("src-129", 0, torch.float64, attn_hook=lambda q, k, v: (q, k, v))
    assert all(np.array_equal(run[k], ref["utts"][0][k]) for k in run)


@pytest.mark.parametrize("defect", sorted(ac.T2_DEFECTS))
def test_t2_planted_defect_is_rejected(defect):
    what, kw, call, utts = ac.T2_DEFECTS[defect]
    ref = ac.t2_reference(call)
    runs = [ac.t2_oracle(call, b, torch.float64, **kw) if b in utts else None for b in range(len(ref["utts"]))]
    r = ac.ratios(ref, runs, ("enc", "mel_output", "alignments", "stop_logits"))
    print(f"SWEEP-RATIO ar_step defect t2-{defect} {call} " + " ".join(f"{q} {v:.1f}" for q, v in r.items()))
    assert max(r.values()) > 1.0, f"{what}: under the bars {r}"


def test_t2_hooks_that_change_nothing_reproduce_the_reference():
    from oracle import tacotron2_ref as t2
    ref = ac.t2_reference("enc32")
    run = ac.t2_oracle("enc32", 1, torch.float64, hooks=dict(lsa=ac._lsa_hook(None), gates=lambda xg, hg: xg + hg),
                       drop=t2.stream_dropout)
    for k in run:
        np.testing.assert_allclose(run[k], ref["utts"][1][k], rtol=0, atol=1e-12)
