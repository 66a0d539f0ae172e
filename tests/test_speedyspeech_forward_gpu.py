"""SpeedySpeech with given durations on the engine: ``forward`` (the reference's rectangle), ``teacher_forced_batch`` (every
utterance alone) and the evaluator's numbers against tests/golden/speedyspeech_forward.npz, the reference's own run.

Regression bar of ``decoded``: ten times the largest mean L1 of the first green hardware run (4.828e-07, rd / f16x3; the other
three combinations of padding reading and math mode gave 3.4e-07 to 4.7e-07)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import mel_loss_ref as mr
from parakeet_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = [("rd", True), ("dil", False)]
NAMES = ("l1_loss", "ssim_loss", "duration_loss", "loss")
# largest mean |decoded - golden| of the first green hardware run (both padding readings, both math modes)
FIRST_RUN_L1 = 4.828e-07
REGRESSION_BAR = 10 * FIRST_RUN_L1


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(GOLD, "speedyspeech_forward.npz")))


def _model(quirk, seed):
    from parakeet_amd.speedyspeech import SpeedySpeech
    m = SpeedySpeech(vocab_size=70, tone_size=7, same_padding_resets_dilation=quirk, **syn.SPEEDYSPEECH_BAKER)
    m.set_state_dict(syn.speedyspeech_state(seed=seed))
    m.eval()
    return m


def _ragged(g):
    n = [int(v) for v in g["num_phones"]]
    return ([g["text"][b, :n[b]] for b in range(3)], [g["tones"][b, :n[b]] for b in range(3)],
            [g["durations"][b, :n[b]] for b in range(3)])


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("tag,quirk", MODES)
def test_forward_matches_the_reference_rectangle(tag, quirk, mode):
    g = _gold()
    m = _model(quirk, int(g["seed"]))
    m.set_math(mode)
    dec, pred = m.forward(g["text"], g["tones"], g["durations"])
    assert tuple(dec.shape) == g[f"{tag}_decoded"].shape and tuple(pred.shape) == (3, 14)
    err = float(np.abs(dec.numpy() - g[f"{tag}_decoded"]).mean())
    perr = float(np.abs(pred.numpy() - g[f"{tag}_pred_durations"]).max())
    print(f"SWEEP-RATIO speedyspeech forward {tag} {mode} decoded mean L1 {err:.3e} pred_durations max {perr:.3e}")
    assert err < 1e-4 and err < REGRESSION_BAR
    assert perr < 1e-4
    # the leak is there: the short utterance's last frames are the rectangle's, not its own B = 1 result
    L = int(g["num_frames"][0])
    assert np.abs(dec.numpy()[0, L - 2:L] - g[f"{tag}_decoded_b0"][L - 2:L]).mean() > 1e-3


@pytest.mark.parametrize("tag,quirk", MODES)
def test_teacher_forced_batch_is_every_utterance_alone(tag, quirk):
    g = _gold()
    m = _model(quirk, int(g["seed"]))
    texts, tones, durs = _ragged(g)
    mels, preds = m.teacher_forced_batch(texts, durs, tones, return_pred_durations=True)
    for b in range(3):
        assert tuple(mels[b].shape) == g[f"{tag}_decoded_b{b}"].shape
        assert np.abs(mels[b].numpy() - g[f"{tag}_decoded_b{b}"]).mean() < 1e-4
        assert np.abs(preds[b].numpy() - g[f"{tag}_pred_durations_b{b}"]).max() < 1e-4
        one, p1 = m.teacher_forced_batch([texts[b]], [durs[b]], [tones[b]], return_pred_durations=True)
        assert np.array_equal(one[0].numpy(), mels[b].numpy()) and np.array_equal(p1[0].numpy(), preds[b].numpy())
    # forward at B = 1 is the ragged reading
    T = int(g["num_phones"][2])
    dec, pred = m.forward(g["text"][2:, :T], g["tones"][2:, :T], g["durations"][2:, :T])
    assert np.array_equal(dec.numpy()[0], mels[2].numpy()) and np.array_equal(pred.numpy()[0], preds[2].numpy())


def test_own_durations_reproduce_inference_and_no_state_leaks():
    g = _gold()
    m = _model(True, int(g["seed"]))
    texts, tones, _ = _ragged(g)
    before = [x.numpy() for x in m.inference_batch(texts, tones)]
    own = [m.debug_tap(2, b).astype(np.int64) for b in range(3)]
    assert [len(x) for x in before] == [int(d.sum()) for d in own]
    forced = m.teacher_forced_batch(texts, own, tones)
    for b in range(3):
        assert np.array_equal(forced[b].numpy(), before[b])
    m.forward(g["text"], g["tones"], g["durations"])
    m.evaluate_batch(g["text"], g["tones"], g["durations"], g["feats"], g["num_frames"], g["num_phones"])
    after = [x.numpy() for x in m.inference_batch(texts, tones)]
    for b in range(3):
        assert np.array_equal(after[b], before[b])
    with pytest.raises(RuntimeError):                       # a plain encode has no target durations
        m._duration_loss_sums()


@pytest.mark.parametrize("tag,quirk", MODES)
def test_evaluators_match_the_reference(tag, quirk):
    g = _gold()
    m = _model(quirk, int(g["seed"]))
    B, L = 3, int(g["num_frames"].max())
    # bounds: the map's per-pixel bound (4 x the reference's own float32 deviation on this batch's masked pairs,
    # <tag>_ssim_ref_dev) on its mean; the decoder's 1e-4 mel bar on the L1 mean, and through the map's slope on the SSIM term;
    # 1e-4 on the log-durations
    got = m.evaluate_batch(g["text"], g["tones"], g["durations"], g["feats"], g["num_frames"], g["num_phones"])
    want = dict(zip(NAMES, g[f"{tag}_losses"]))
    dec, pred = m.forward(g["text"], g["tones"], g["durations"])
    exact = mr.evaluate(dec.numpy(), pred.numpy(), g["durations"], g["feats"], g["num_frames"], g["num_phones"])
    print(f"SWEEP-RATIO speedyspeech evaluate_batch {tag} " + " ".join(f"{k} {got[k]:.6f} ({got[k] - want[k]:+.2e})" for k in NAMES))
    assert abs(got["l1_loss"] - exact["l1_loss"]) <= 1e-6 * exact["l1_loss"]           # the L1 sum's bound
    dev = float(g[f"{tag}_ssim_ref_dev"])
    assert abs(got["ssim_loss"] - exact["ssim_loss"]) <= 4 * dev                      # the map's bound, on its mean
    assert abs(got["duration_loss"] - exact["duration_loss"]) <= 1e-6
    assert abs(got["l1_loss"] - want["l1_loss"]) < 1e-4 and abs(got["duration_loss"] - want["duration_loss"]) < 1e-4
    assert abs(got["ssim_loss"] - want["ssim_loss"]) < 1e-4 + 4 * dev
    assert got["loss"] == got["l1_loss"] + got["ssim_loss"] + got["duration_loss"]
    texts, tones, durs = _ragged(g)
    targets = [g["feats"][b, :int(g["num_frames"][b])] for b in range(B)]
    per = m.evaluate_per_utterance(texts, durs, targets, tones)
    for b in range(B):
        wb = dict(zip(NAMES, g[f"{tag}_losses_b{b}"]))
        assert abs(per[b]["l1_loss"] - wb["l1_loss"]) < 1e-4 and abs(per[b]["duration_loss"] - wb["duration_loss"]) < 1e-4
        assert abs(per[b]["ssim_loss"] - wb["ssim_loss"]) < 1e-4 + 4 * float(g[f"{tag}_ssim_ref_dev_b{b}"])
        alone = m.evaluate_per_utterance([texts[b]], [durs[b]], [targets[b]], [tones[b]])[0]
        assert alone == per[b]                               # bit-identical in any batch
    with pytest.raises(ValueError, match="pair 1"):
        m.evaluate_per_utterance(texts, durs, [targets[0], targets[1][:-1], targets[2]], tones)


def test_errors():
    from parakeet_amd import _capi
    g = _gold()
    m = _model(True, int(g["seed"]))
    texts, tones, durs = _ragged(g)
    bad = [d.copy() for d in durs]
    bad[1][2] = -1
    with pytest.raises(ValueError, match="negative"):
        m.teacher_forced_batch(texts, bad, tones)
    with pytest.raises(ValueError, match="durations"):
        m.teacher_forced_batch(texts, [durs[0], durs[1][:-1], durs[2]], tones)
    with pytest.raises(ValueError):
        m.forward(g["text"], g["tones"], g["durations"][:, :-1])
    # frame_lens below the sum of durations, through the C ABI
    m._finalize()
    lib = m._ctx.lib
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    tx, ds = np.ascontiguousarray(texts[0]), np.ascontiguousarray(durs[0])
    lens, out = np.array([len(tx)], np.int32), np.zeros(1, np.int32)
    short = np.array([int(ds.sum()) - 1], np.int32)
    rc = lib.pk_ss_encode_given(m._h, tx.ctypes.data_as(i64p), None, lens.ctypes.data_as(i32p), ds.ctypes.data_as(i64p),
                                short.ctypes.data_as(i32p), 1, out.ctypes.data_as(i32p))
    assert rc == -1 and b"frame_lens" in lib.pk_last_error()
    exact = np.array([int(ds.sum()) + 3], np.int32)
    _capi.check(lib.pk_ss_encode_given(m._h, tx.ctypes.data_as(i64p), None, lens.ctypes.data_as(i32p), ds.ctypes.data_as(i64p),
                                       exact.ctypes.data_as(i32p), 1, out.ctypes.data_as(i32p)))
    assert out[0] == exact[0]
    host = np.full(len(tx), np.nan, np.float32)
    _capi.check(lib.pk_ss_pred_durations(m._h, _capi.fptr(host), _capi.PK_HOST_IO))
    assert np.isfinite(host).all()
    sums = np.full(1, np.nan)
    _capi.check(lib.pk_ss_duration_loss(m._h, sums.ctypes.data_as(C.c_void_p), _capi.PK_HOST_IO))
    want = mr.huber(host, np.log(np.maximum(ds, 1))).sum()
    assert abs(sums[0] - want) <= 1e-6 * want
    # ... and after a plain encode there is nothing to compare with
    m.encode_batch([texts[0]])
    rc = lib.pk_ss_duration_loss(m._h, sums.ctypes.data_as(C.c_void_p), _capi.PK_HOST_IO)
    assert rc == -6 and lib.pk_last_error()
