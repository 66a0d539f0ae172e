"""The speaker-encoder kernels (csrc/spk.hip: ``k_spk_pad_in``, ``k_spk_lstm_rec`` in its four instantiations, ``k_spk_head``)
over every admitted hidden size, initial states, tile and length edges, input widths and head sizes, in both maths, through
``LSTMSpeakerEncoder`` against the float64 oracle under the bar of tests/spk_lstm_cases.py (4 x the float32 oracle's own error,
from the references alone).  ``SWEEP-RATIO spk_lstm <case> <math> <quantity> <error / bar>`` before every assertion.

Groups A - E and the small call of G: per-partial embeddings (and, in E, the utterance embeddings of a ragged
``embed_utterances``) under the bar.  F: bit-exact properties.  G: the size refusal.

Measured on an MI355X (largest error / bar of any case of the group):

    group                                   f16x3                        f32
    A  every hidden size                    0.33 (H 512)                 0.41 (H 480)
    B  initial states                       0.36 (H 256, 2 layers, T 8)  0.76 (H 512, 2 layers, T 2)
    C  tile and length edges                0.31 (H 64, P 1, T 160)      0.47 (H 320, P 32, T 1)
    D  n_mels 1, 32, 33, 257, 512           0.32 (n_mels 1)              0.34 (n_mels 33)
    D  n_mels 513, 4096 (k_spk_proj_wide)   0.15 (n_mels 513)            0.19 (n_mels 513)
    E  head, per partial and per utterance  0.41 (E-zero, utterances)    0.41 (E-zero, partials)
    G  the small call after the refusal     0.31                         0.31

Found and fixed in csrc/spk.hip.  ``k_spk_lstm_rec`` seeded its accumulators with the step's input projection xg, so each of the
H / 2 (f32) or 3 H / 16 (f16x3) accumulation steps of h(t-1) . W_hh^T rounded at the magnitude of xg + partial sum instead of the
partial sum's.  "G-small" in f32 was at 1.18 x its bar (error 9.80e-8, bar 8.30e-8; 3.0e-8 after one step, where nothing is
accumulated, 9.6e-8 after two), and a float32 restatement that seeds its sum the same way reproduces it (9.2e-8 against 3.4e-8
unseeded).  The accumulators now start at zero and xg is added once behind the matrix loop: "G-small" 0.31 in both maths, the
largest f32 ratio of group A 0.74 -> 0.41, of C 0.97 -> 0.47, of D (n_mels <= 257) 0.94 -> 0.34.

Found and fixed, second: "D-h32-m4096" was at 2.61 (f32) / 3.14 (f16x3) x its bar, error 4.51e-6 / 5.42e-6 against 1.73e-6.  Not the
recurrence: the layer-0 projection was one pass of the tile GEMM, which sums its K = 4096 products in one float32 accumulator,
k ascending.  With inputs exp(N(-2, 2)) the partial sums reach 50 - 100 and every step rounds at that magnitude; a float32
restatement with the projection summed one k at a time gives 4.24e-6 at T = 3 and 1.77e-6 at T = 1 (the engine: 4.52e-6 and
1.78e-6).  Above 512 mel channels layer 0 is now projected by ``k_spk_proj_wide`` with float64 accumulators: 0.04 / 0.03.  The
cases n_mels 512 and 513 stand on the two sides of that threshold (0.26 / 0.23 and 0.19 / 0.15).
"""
import functools

import numpy as np
import pytest

import spk_lstm_cases as sc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def _model(name):
    """The engine model of a case (kept for the case's second math)."""
    from parakeet_amd.lstm_speaker_encoder import LSTMSpeakerEncoder
    m = LSTMSpeakerEncoder(**sc.config(name))
    m.set_state_dict(sc.state(name))
    m.eval()
    return m


def _utterances(name):
    x, _ = sc.inputs(name)
    cu = sc.bounds(name)
    return [x[a:b] for a, b in zip(cu[:-1], cu[1:])]


@pytest.mark.parametrize("math", sc.MATHS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_spk_lstm_sweep(name, math):
    """Groups A - E and G-small under their bars."""
    c, ref = sc.CASE[name], sc.reference(name)
    x, states = sc.inputs(name)
    m = _model(name)
    m.set_math(math)
    got = {"seq": m.embed_sequences(x, initial_states=states).cpu().numpy()}
    if c["utterances"] is not None:
        got["utt"] = m.embed_utterances(_utterances(name)).cpu().numpy()
    errs = {}
    for k, g in got.items():
        assert g.shape == ref[k].shape and np.isfinite(g).all(), k
        errs[k] = sc.error(g, ref[k])
        print(f"SWEEP-RATIO spk_lstm {name} {math} {k} {errs[k] / ref['bar'][k]:.4f}   (error {errs[k]:.3e}, bar {ref['bar'][k]:.3e})")
    for k in got:
        assert errs[k] <= ref["bar"][k], f"{name} {math} {k}: error {errs[k]:.3e} above the bar {ref['bar'][k]:.3e}"
    if name == "E-zero":
        assert not got["seq"][sc.ZERO_ROW].any()           # the all-zero ReLU row stays the zero vector under the clamp
        assert got["seq"][sc.ZERO_ROW - 1].any() and got["seq"][sc.ZERO_ROW + 1].any()


# ---- F: bit-exact properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", sc.MATHS)
@pytest.mark.parametrize("name", ("B-h96-l2-t3", "B-h288-l3-t2"))
def test_zero_states_are_no_states(name, math):
    """Zero arrays as ``initial_states`` give the bits of ``initial_states=None``: the row scale of a zero row is a power of two
    (exact on the way in and out) and every product with it is zero."""
    c = sc.CASE[name]
    x, _ = sc.inputs(name)
    m = _model(name)
    m.set_math(math)
    zeros = np.zeros((c["layers"], c["P"], c["H"]), dtype=np.float32)
    a = m.embed_sequences(x, initial_states=(zeros, zeros.copy())).cpu().numpy()
    b = m.embed_sequences(x).cpu().numpy()
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("math", sc.MATHS)
@pytest.mark.parametrize("name", ("B-h96-l2-t3", "B-h512-l3-t2"))
def test_states_batch_invariance(name, math):
    """With ``h0`` rows of magnitudes over five decades, one all-zero row and one of magnitude 1e-30, each partial embedded
    alone equals its row of the batched call bit for bit: the exponent of ``h0`` is the row's own, not the tile's."""
    c = sc.CASE[name]
    x, _ = sc.inputs(name)
    h0, c0 = sc.initial_states(c["layers"], c["P"], c["H"], 3000 + c["seed"], special_rows=True)
    assert not h0[:, 1].any() and 0.0 < np.abs(h0[:, 2]).max() <= 1e-30
    mags = np.abs(h0).max(-1)
    assert mags[mags > 1e-20].max() / mags[mags > 1e-20].min() > 1e4
    m = _model(name)
    m.set_math(math)
    together = m.embed_sequences(x, initial_states=(h0, c0)).cpu().numpy()
    assert np.isfinite(together).all()
    for p in range(c["P"]):
        alone = m.embed_sequences(x[p:p + 1], initial_states=(np.ascontiguousarray(h0[:, p:p + 1]),
                                                               np.ascontiguousarray(c0[:, p:p + 1]))).cpu().numpy()
        assert np.array_equal(alone[0], together[p]), f"partial {p} (|h0| up to {mags[:, p].max():.1e}) depends on its batch"


@pytest.mark.parametrize("math", sc.MATHS)
@pytest.mark.parametrize("name", ("E-h32-o288", "E-h512-o4096", "E-zero"))
def test_ragged_utterances_equal_single_calls(name, math):
    """``embed_utterances`` on the ragged list of group E equals per-utterance ``embed_utterance`` calls bit for bit."""
    m = _model(name)
    m.set_math(math)
    utts = _utterances(name)
    together = m.embed_utterances(utts).cpu().numpy()
    for u, b in enumerate(utts):
        assert np.array_equal(together[u], m.embed_utterance(b).cpu().numpy()), f"utterance {u} ({len(b)} partials) differs"


# ---- G: the size refusal -------------------------------------------------------------------------------------------------------
def test_oversized_call_is_refused_before_any_launch():
    """One partial of 2^30 / 4H + 1 frames at H = 512 raises the wrapper's error for PK_EUNSUPPORTED with no kernel launched;
    a small call on the same model afterwards is right."""
    from parakeet_amd.runtime import Context
    name = "G-small"
    c = sc.CASE[name]
    assert sc.REFUSED_T == 524289 and c["H"] == 512 and c["n_mels"] == 1
    m = _model(name)
    m.set_math("f16x3")
    big = np.full((1, sc.REFUSED_T, 1), 0.1, dtype=np.float32)
    ctx = Context.get()
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        with pytest.raises(NotImplementedError, match="exceed"):
            m.embed_sequences(big)
        ran = {k: n for k, (n, _) in ctx.prof_dump().items() if n > 0}
    finally:
        ctx.prof_enable(False)
    assert not ran, ran
    x, _ = sc.inputs(name)
    ref = sc.reference(name)
    for math in sc.MATHS:
        m.set_math(math)
        err = sc.error(m.embed_sequences(x).cpu().numpy(), ref["seq"])
        print(f"SWEEP-RATIO spk_lstm {name} after-refusal {math} seq {err / ref['bar']['seq']:.4f}")
        assert err <= ref["bar"]["seq"], f"{math}: error {err:.3e} above the bar {ref['bar']['seq']:.3e}"
