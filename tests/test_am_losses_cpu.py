"""The float64 restatement of the acoustic models' criteria (tests/am_loss_ref.py) against what the reference's own
classes gave in float32 (tests/golden/am_losses.npz, tools/make_golden_am_losses.py), the docstring tables of the guide,
and the per-entry bound of the GPU tests held against the reference's own fp32 formula."""
import functools
import os
import re

import numpy as np
import pytest

import am_loss_cases as ac
import am_loss_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-6

TABLE_5_5, TABLE_3_6 = ac.TABLE_5_5, ac.TABLE_3_6


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "am_losses.npz")))


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert (np.abs(got - want) <= REL * np.abs(want)).all(), (got, want)


def test_cases_cover_what_the_issue_lists():
    modes = lambda cs: {(um, uw) for um, uw, *_ in cs.values()}   # noqa: E731
    assert modes(ac.FS2_CASES) == modes(ac.TTS_CASES) == {(True, False), (False, False), (False, True)}
    assert any(not after for *_, after in ac.FS2_CASES.values())
    assert {pw for *_, pw in ac.TTS_CASES.values()} == {1.0, 5.0}
    assert ac.LOSS_TYPES == ("L1", "L2", "L1+L2")
    assert {(s, g) for s, g, _ in ac.TACO_CASES.values()} == {(True, False), (False, False), (False, True), (True, True)}
    assert any(i == 1 and o == 1 for i, o in zip(ac.ILENS, ac.OLENS)) and len(set(ac.OLENS)) == len(ac.OLENS)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "am_losses.npz")) < 32 * 1024


@pytest.mark.parametrize("name", list(ac.FS2_CASES))
def test_fastspeech2_loss(name):
    um, uw, with_after = ac.FS2_CASES[name]
    x = ac.fs2_inputs()
    if not with_after:
        x["after_outs"] = None
    _close(ar.fastspeech2_loss(**x, use_masking=um, use_weighted_masking=uw), _gold()[name])


@pytest.mark.parametrize("name", list(ac.DUR_CASES))
def test_duration_predictor_loss(name):
    offset, seed = ac.DUR_CASES[name]
    _close(ar.duration_predictor_loss(*ac.dur_inputs(seed), offset=offset), _gold()[name])


@pytest.mark.parametrize("name", list(ac.TTS_CASES))
def test_transformer_tts_loss_and_the_evaluators_totals(name):
    um, uw, pw = ac.TTS_CASES[name]
    l1, l2, bce = ar.transformer_tts_loss(**ac.tts_inputs(), use_masking=um, use_weighted_masking=uw, bce_pos_weight=pw)
    _close([l1, l2, bce], _gold()[name])
    _close([ar.transformer_tts_total(l1, l2, bce, t) for t in ac.LOSS_TYPES], _gold()[name + "_totals"])
    with pytest.raises(ValueError):
        ar.transformer_tts_total(l1, l2, bce, "L3")


def test_the_flag_pair_assertion():
    with pytest.raises(AssertionError):
        ar.transformer_tts_loss(**ac.tts_inputs(), use_masking=True, use_weighted_masking=True)
    x = ac.fs2_inputs()
    with pytest.raises(AssertionError):
        ar.fastspeech2_loss(**x, use_masking=True, use_weighted_masking=True)


@pytest.mark.parametrize("name", list(ac.GA_CASES))
def test_guided_attention_losses(name):
    _, sigma, alpha, heads = ac.GA_CASES[name]
    _close(ar.guided_attention_loss_tts(ac.attention(31, heads), ac.ILENS, ac.OLENS, sigma, alpha), _gold()[name])


@pytest.mark.parametrize("name", list(ac.TACO_CASES))
def test_tacotron2_loss(name):
    stop, guided, sigma = ac.TACO_CASES[name]
    got = ar.tacotron2_loss(**ac.taco_inputs(), use_stop_token_loss=stop, use_guided_attention_loss=guided, sigma=sigma)
    want = {k.split("/")[1]: v for k, v in _gold().items() if k.startswith(name + "/")}
    assert set(got) == set(want) == {"loss", "mel_loss", "post_mel_loss"} | ({"stop_loss"} if stop else set()) | (
        {"guided_attn_loss"} if guided else set())
    for k in want:
        _close(got[k], want[k])


def test_attention_guide_and_guided_attention_loss():
    x = ac.taco_inputs()
    att = x["attention_weights"]
    W = ar.attention_guide(ac.OLENS, ac.ILENS, att.shape[1], att.shape[2], ac.GUIDE_G)
    want = _gold()["attention_guide"].astype(np.float64)
    assert W.shape == want.shape and np.abs(W - want).max() <= ar.guide_entry_bound(ac.GUIDE_G)
    assert (W[1, 1:] == 0).all() and (W[1, :, 1:] == 0).all()          # the single-frame, single-token utterance
    _close(ar.guided_attention_loss(att, ac.OLENS, ac.ILENS, ac.GUIDE_G), _gold()["guided_attention_loss"])


def test_the_guide_reproduces_both_docstring_tables():
    for name, table in (("table_5_5", TABLE_5_5), ("table_3_6", TABLE_3_6)):
        ilen, olen, sigma = ac.TABLES[name]
        w = ar.guide(ilen, olen, sigma)
        assert w.shape == (olen, ilen) == np.shape(table)
        assert np.array_equal(np.round(w, 4), np.asarray(table))
        assert np.abs(w - _gold()[name]).max() <= ar.guide_entry_bound(sigma)
        # the restatement in fp32 is the reference's arithmetic: the two differ by their libraries' expf alone, each within
        # 1 ulp of a value below 1 (ulp <= u)
        assert np.abs(ar.guide_f32(ilen, olen, sigma).astype(np.float64) - _gold()[name]).max() <= 2 * ar.U


@pytest.mark.parametrize("sigma", [0.05, 0.2, 0.4, 1.0])
def test_the_per_entry_bound_holds_for_the_references_own_fp32_formula(sigma):
    worst = 0.0
    for ilen, olen in ((5, 5), (3, 6), (17, 33), (65, 129), (129, 640), (7, 1000), (1, 1), (1, 9), (9, 1)):
        exact = ar.guide(ilen, olen, sigma)
        for recip in (False, True):
            err = np.abs(ar.guide_f32(ilen, olen, sigma, recip).astype(np.float64) - exact).max()
            worst = max(worst, err / ar.guide_entry_bound(sigma))
    print(f"SWEEP-RATIO guide fp32 formula sigma {sigma} worst {worst:.4f}")
    assert worst <= 1.0


def test_the_bound_reads_the_kernels_constants():
    from parakeet_amd import _capi
    header = open(os.path.join(ROOT, "parakeet_amd", "csrc", "pk_seq_loss.h")).read()
    val = lambda n: int(re.search(rf"#define {n} (\d+)", header).group(1))   # noqa: E731
    assert val("PK_SEQ_LOSS_F32_CHAIN") == _capi.PK_SEQ_LOSS_F32_CHAIN
    assert val("PK_SEQ_LOSS_GUIDE_ROWS") == _capi.PK_SEQ_LOSS_GUIDE_ROWS
    assert val("PK_SEQ_LOSS_GUIDE_COLS") == _capi.PK_SEQ_LOSS_GUIDE_COLS
    assert 256 * val("PK_SEQ_LOSS_VEC") * val("PK_SEQ_LOSS_PAIR_ITERS") == _capi.PK_SEQ_LOSS_PAIR_TILE
    assert ar.guided_sums_bound(0.4, 1.0, 0.0, 0) == 2 * (3.1 / 0.4 + 6.2) * 2.0 ** -24


def test_forward_targets_of_transformer_tts():
    labels, olens, ilens, n = ar.transformer_tts_forward_targets([3, 5], [4, 7], 7, r=1)
    assert np.array_equal(labels, [[0, 0, 0, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 1]]) and n == 7
    assert olens.tolist() == [4, 7] and ilens.tolist() == [4, 6]
    labels, olens, ilens, n = ar.transformer_tts_forward_targets([3, 5], [4, 7], 7, r=2)
    assert olens.tolist() == [4, 6] and n == 6
    assert np.array_equal(labels, [[0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 0, 1]])


def test_new_names_are_exposed():
    import parakeet_amd.fastspeech2 as fs2
    import parakeet_amd.losses as losses
    import parakeet_amd.tacotron2 as taco
    import parakeet_amd.transformer_tts as tts
    for name in ("pair_loss_sums", "bce_with_logits_sums", "guided_attention_sums", "attention_guide", "guided_attention_loss"):
        assert callable(getattr(losses, name)), name
    assert "masked_softmax_with_cross_entropy" in losses.__doc__ and not hasattr(losses, "masked_softmax_with_cross_entropy")
    assert callable(fs2.FastSpeech2Loss) and callable(fs2.DurationPredictorLoss) and callable(taco.Tacotron2Loss)
    for name in ("TransformerTTSLoss", "GuidedAttentionLoss", "GuidedMultiHeadAttentionLoss"):
        assert callable(getattr(tts, name)), name
    for cls in (fs2.FastSpeech2, tts.TransformerTTS, taco.Tacotron2):
        assert callable(cls.evaluate_batch) and callable(cls.evaluate_per_utterance)
    with pytest.raises(AssertionError):
        fs2.FastSpeech2Loss(use_masking=True, use_weighted_masking=True)
    with pytest.raises(AssertionError):
        tts.TransformerTTSLoss(use_masking=True, use_weighted_masking=True)
