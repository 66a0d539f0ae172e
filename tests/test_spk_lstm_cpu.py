"""The inputs and the bars of the speaker-encoder sweep (tests/spk_lstm_cases.py) are worth something: no GPU.

Bars.  Every case has a bar that comes out of the oracle's own float32 error (two summation orders) and nothing else.

Second statement.  ``restated`` (plain numpy, float64) reproduces ``ge2e_ref`` for every case.

Planted defects.  Each way the kernels could be subtly wrong (``DEFECTS``) moves the float64 result of every case it applies to
by at least 8 x that case's bar.  ``layer0_states`` and ``c0_last_block_zero`` apply to group B alone (the cases with initial
states, T <= 8): an LSTM forgets its state, and the group is kept that short so that the states are still visible.

The extension of ``ge2e_ref`` (``dtype``, the per-layer h sequences) is pinned here as well.

``SPK-LSTM-E32`` lines give e32 / peak / bar per case; ``SWEEP-RATIO spk_lstm defect`` lines the shift of a defect / bar.
"""
import numpy as np
import pytest
import torch

import ge2e_ref
import spk_lstm_cases as sc


def test_case_table():
    """The table holds what the sweep is meant to cover."""
    by = {g: [c for c in sc.CASES if c["group"] == g] for g in sc.GROUPS}
    assert [c["H"] for c in by["A"]] == list(range(32, 513, 32))
    assert all(c["layers"] == 2 and c["T"] == 12 and c["P"] == 33 and c["n_mels"] == 40 and not c["states"] for c in by["A"])
    assert {(c["H"], c["layers"], c["T"]) for c in by["B"]} == {(H, L, T) for H in (32, 96, 256, 288, 512) for L in (2, 3)
                                                                 for T in (1, 2, 3, 8)}
    assert all(c["states"] and c["P"] == 33 for c in by["B"])
    for H in (64, 320):
        cs = [c for c in by["C"] if c["H"] == H]
        assert all(c["layers"] == 3 for c in cs)
        assert {c["P"] for c in cs} == {1, 31, 32, 33, 64, 65, 97} and {c["T"] for c in cs} == {1, 2, 160}
    assert {(c["H"], c["n_mels"]) for c in by["D"]} == {(288, 1), (288, 32), (288, 33), (288, 257), (32, 4096), (288, 512),
                                                             (288, 513)}
    assert all(c["P"] == 5 and c["T"] == 3 for c in by["D"])
    assert {(c["H"], c["O"]) for c in by["E"] if c["head"] == "xavier"} == {(H, O) for H in (32, 512) for O in (32, 288, 4096)}
    assert all(c["utterances"] == (1, 2, 70) for c in by["E"] if c["head"] == "xavier")
    assert all(c["O"] == 2 * c["H"] and c["head"] == "identity" for g in "ABCD" for c in by[g])


@pytest.mark.parametrize("name", sc.NAMES)
def test_reference_and_bar(name):
    c, ref = sc.CASE[name], sc.reference(name)
    assert ref["seq"].shape == (c["P"], c["O"])
    if c["utterances"] is not None:
        assert ref["utt"].shape == (len(c["utterances"]), c["O"])
    for k in ref["bar"]:
        e32, peak, bar = ref["e32"][k], ref["peak"][k], ref["bar"][k]
        print(f"SPK-LSTM-E32 {name} {k} e32 {e32:.3e} peak {peak:.3f} bar {bar:.3e}")
        assert bar == 4.0 * max(e32, sc.ulp32(peak))
        assert np.isfinite(e32) and e32 > 0.0 and 0.0 < peak <= 1.0, (k, e32, peak)
        assert bar < 1e-5, (k, bar)      # an order under the 1e-4 contract of tests/test_speaker_encoder_gpu.py
    if c["head"] == "identity":
        # the probe is h(T) of the last layer, element by element, up to its norm
        h = ref["h"]
        want = np.concatenate([np.maximum(h, 0.0), np.maximum(-h, 0.0)], 1) / np.linalg.norm(h, axis=1, keepdims=True)
        np.testing.assert_allclose(ref["seq"], want, rtol=0, atol=1e-14)


def test_zero_relu_case_shows_in_the_reference():
    """E-zero: one partial of the second utterance has an all-zero ReLU output, every other partial a live one; the reference
    embeds it as the zero vector (the 1e-12 clamp) and its utterance as the normalised mean of the others."""
    ref = sc.reference("E-zero")
    norms = np.linalg.norm(ref["seq"], axis=1)
    assert norms[sc.ZERO_ROW] == 0.0 and not ref["seq"][sc.ZERO_ROW].any()
    others = np.delete(norms, sc.ZERO_ROW)
    np.testing.assert_allclose(others, 1.0, rtol=0, atol=1e-12)
    cu = sc.bounds("E-zero")
    assert cu[1] <= sc.ZERO_ROW < cu[2]
    live = [r for r in range(cu[1], cu[2]) if r != sc.ZERO_ROW]
    mean = ref["seq"][live].sum(0)
    np.testing.assert_allclose(ref["utt"][1], mean / np.linalg.norm(mean), rtol=0, atol=1e-14)
    dead = [o for o in range(sc.CASE["E-zero"]["O"]) if o not in sc.ZERO_LIVE]
    assert not ref["seq"][:, dead].any()


@pytest.mark.parametrize("name", sc.NAMES)
def test_second_statement_agrees_with_the_oracle(name):
    ref, got = sc.reference(name), sc.restated(name)
    for k in ref["bar"]:
        err = sc.error(got[k], ref[k])
        print(f"SWEEP-RATIO spk_lstm second statement {name} {k} {err / ref['bar'][k]:.3e}")
        assert err < 1e-6 * ref["bar"][k], (k, err)


@pytest.mark.parametrize("defect", sorted(sc.DEFECTS))
def test_planted_defect_is_rejected(defect):
    names = [n for n in sc.NAMES if sc.applicable(n, defect)]
    assert names, defect
    if defect in ("layer0_states", "c0_last_block_zero"):
        assert all(sc.CASE[n]["group"] == "B" for n in names) and len(names) == 40
    shifts = {name: sc.defect_shift(name, defect) for name in names}
    for name, shift in shifts.items():
        print(f"SWEEP-RATIO spk_lstm defect {defect} {name} {shift:.1f}")
    print(f"SWEEP-RATIO spk_lstm defect {defect} smallest of {len(names)} cases {min(shifts.values()):.1f}")
    for name, shift in shifts.items():
        assert shift >= sc.DEFECT_MARGIN, f"{sc.DEFECTS[defect]}: {name} moves by {shift:.2f} x its bar"


def test_every_group_meets_its_defects():
    """Which defects each group is a guard against (from ``applicable`` alone)."""
    def groups(defect):
        return {sc.CASE[n]["group"] for n in sc.NAMES if sc.applicable(n, defect)}
    assert groups("second_block_stale") >= {"A", "B", "C", "D", "E"}
    assert groups("h_single_fp16") == {"A", "B", "C"}
    assert groups("tail_row_neighbour") >= {"A", "B", "C"}
    assert groups("o_tail_dropped") >= {"E"} and groups("mean_before_normalise") == {"E"}
    assert groups("pad_column_live") >= {"A", "D"}
    # both UBW instantiations meet the states defects
    assert {sc.CASE[n]["H"] > 256 for n in sc.NAMES if sc.applicable(n, "layer0_states")} == {True, False}


def test_ge2e_ref_dtype_and_layers():
    """``dtype`` defaults to float64 and changes nothing there; float32 is a float32 evaluation; ``return_layers`` returns every
    layer's h sequence, the last step of the last one being the returned h(T)."""
    name = "B-h96-l3-t3"
    c, st = sc.CASE[name], sc.state(name)
    x, states = sc.inputs(name)
    h = ge2e_ref.lstm_last_hidden(st, x, c["layers"], states)
    h2, layers = ge2e_ref.lstm_last_hidden(st, x, c["layers"], states, dtype=torch.float64, return_layers=True)
    assert h.dtype == torch.float64 and torch.equal(h, h2)
    assert len(layers) == c["layers"] and all(s.shape == (c["P"], c["T"], c["H"]) for s in layers)
    assert torch.equal(layers[-1][:, -1], h)
    h32 = ge2e_ref.lstm_last_hidden(st, x, c["layers"], states, dtype=torch.float32)
    assert h32.dtype == torch.float32
    assert 0.0 < float((h32.double() - h).abs().max()) < 1e-5
    e = ge2e_ref.embed_sequences(st, x, c["layers"], states)
    e2, layers2 = ge2e_ref.embed_sequences(st, x, c["layers"], states, return_layers=True)
    assert torch.equal(e, e2) and torch.equal(layers2[0], layers[0])
    assert ge2e_ref.embed_sequences(st, x, c["layers"], states, dtype=torch.float32).dtype == torch.float32
