"""The inputs and the bars of the FFT-stack sweep (tests/fft_stack_cases.py) are worth something: no GPU.

Input conditions.  The sweep drives the attention kernels through whole models, so what the running maximum, the rescale of O
and the key mask are worth depends on the attention the models produce.  Asserted from the float64 oracle alone, for every model
at query gains 8 and 32: the median row peak of layer 0 of either stack, and for the encoder, whose input the seeds control, a row
per long utterance whose largest weight lies outside the first key tile and a row per utterance with a partial last key tile
that puts weight on it.

Planted defects.  A second float64 statement of the encoder stack (``restated_hs``) reproduces the oracle, and each of seven
ways the kernels could be subtly wrong moves the encoder tap of its target case above that case's bar.

``SWEEP-RATIO`` lines give error / bar; ``FFT-STACK-E32`` lines the table of DESIGN.md.
"""
import numpy as np
import pytest

import fft_stack_cases as fc


@pytest.mark.parametrize("gain", fc.GAINS)
@pytest.mark.parametrize("name", fc.NAMES)
def test_reference_and_bar(name, gain):
    """The references are what they claim: integer durations of one frame per token (both stacks see the chosen lengths), a bar
    that comes out of the oracle's own float32 error and nothing else."""
    ref = fc.reference(name, gain)
    for T, d, hs, zs in zip(fc.LENGTHS, ref["d"], ref["hs"], ref["zs"]):
        np.testing.assert_array_equal(d, np.ones(T))
        assert hs.shape == zs.shape == (T, fc.MODEL[name]["adim"])
    for tap in ("hs", "zs"):
        e32, peak, bar = ref["e32"][tap], ref["peak"][tap], ref["bar"][tap]
        print(f"FFT-STACK-E32 {fc.case_id(name, gain)} {tap} e32 {e32:.3e} peak {peak:.3f} bar {bar:.3e}")
        assert bar == 4.0 * max(e32, fc.ulp32(peak))
        assert np.isfinite(e32) and e32 > 0.0 and peak > 0.0, (tap, e32, peak)


# The one stack that cannot meet the medians at the gains the sweep uses: layer 0 of a post-norm encoder sees the embeddings
# without a LayerNorm in front (rms 0.7 instead of 1), so a gain gives logits half as wide as in every other stack (0.18 / 0.68 at
# gains 8 / 32).  It is held to floors of its own, so that a change of the inputs is still caught; its decoder, fed by the
# encoder's last LayerNorm, meets the common bounds (0.71 / 0.995) and runs the same kernels.
MEDIAN_FLOOR = {("a384h2post", "enc"): {8: 0.15, 32: 0.6}}


@pytest.mark.parametrize("gain", (8, 32))
@pytest.mark.parametrize("name", fc.NAMES)
def test_input_conditions(name, gain):
    cond = fc.input_conditions(fc.reference(name, gain))
    for stack in ("enc", "dec"):
        median, no_far, no_tail = cond[stack]
        print(f"FFT-STACK-INPUT {fc.case_id(name, gain)} {stack} median row peak {median:.3f}, lengths without a row that looks "
              f"beyond key tile 0: {no_far}, without {fc.TAIL_WEIGHT_MIN} on the last partial tile: {no_tail}")
        assert median >= MEDIAN_FLOOR.get((name, stack), fc.PEAK_MEDIAN_MIN)[gain], (stack, median)
    # per utterance, in the encoder (what the seeds were searched for; the decoder's figures are a record)
    _, no_far, no_tail = cond["enc"]
    assert not no_far, f"no row of the utterances of {no_far} rows looks beyond key tile 0"
    assert not no_tail, f"no row of the utterances of {no_tail} rows puts {fc.TAIL_WEIGHT_MIN} on the last partial tile"


def test_attention_helper_matches_the_statistics():
    """``attention_layer0`` returns what the statistics were taken from: rows that sum to one, the same peaks."""
    name, gain, b = "a128h2", 8, fc.LENGTHS.index(33)
    a = fc.attention_layer0(name, gain, b)
    assert a.shape == (2, 33, 33)
    np.testing.assert_allclose(a.sum(-1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(a.max(-1), fc.reference(name, gain)["enc"][b]["peak"])


# (model, gain) the defects are planted in: the smallest model, a model of the widest head at the widest logits, and -- for the
# dropped lo half of K, whose effect grows with the logits -- the recipe's shape at gain 1, where it is smallest
TARGETS = (("a64h1", 8), ("a192h1", 32), ("a384h2", 1))


@pytest.mark.parametrize("name,gain", TARGETS, ids=[fc.case_id(*t) for t in TARGETS])
def test_second_statement_agrees_with_the_oracle(name, gain):
    ref = fc.reference(name, gain)
    for reverse in (False, True):
        hs = fc.restated_hs(name, gain, reverse=reverse)
        err = fc.tap_error(hs[::-1] if reverse else hs, ref["hs"])
        print(f"SWEEP-RATIO fft_stack second statement {fc.case_id(name, gain)} reverse={reverse} {err / ref['bar']['hs']:.3e}")
        assert err < 1e-6 * ref["bar"]["hs"], err


@pytest.mark.parametrize("defect", sorted(fc.DEFECTS))
def test_planted_defect_is_rejected(defect):
    for name, gain in TARGETS:
        if name == "a384h2" and defect != "k_single_fp16":
            continue
        ref = fc.reference(name, gain)
        err = fc.tap_error(fc.restated_hs(name, gain, defect), ref["hs"])
        print(f"SWEEP-RATIO fft_stack defect {defect} {fc.case_id(name, gain)} hs {err / ref['bar']['hs']:.1f}")
        assert err > ref["bar"]["hs"], f"{fc.DEFECTS[defect]}: error {err:.3e} under the bar {ref['bar']['hs']:.3e}"
