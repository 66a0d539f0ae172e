"""The per-utterance sums of csrc/seq_loss.hip (pk_guided_attn_run, pk_pair_loss_run, pk_bce_logits_run) against the float64
restatement of tests/am_loss_ref.py, and the criteria built on them against the reference's own numbers
(tests/golden/am_losses.npz).

Bounds.  Guided sums: absolute, derived at the top of tests/am_loss_ref.py from the kernel's operation order and
PK_SEQ_LOSS_F32_CHAIN.  Pair sums: 1e-6 relative (a float32 difference, or its exact square, summed in float64: the bar of
tests/test_mel_loss_gpu.py).  BCE sums: 1e-6 relative to the same formula in float64.  Criteria: 2e-6 relative (the golden's
float32 plus the engine's 1e-6).  ``SWEEP-RATIO`` lines give error / bound."""
import functools
import os

import numpy as np
import pytest
import torch

import am_loss_cases as ac
import am_loss_ref as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edges(e):
    return (1, 2, e - 1, e, e + 1, 2 * e + 1)


@functools.lru_cache(maxsize=None)
def _consts():
    from parakeet_amd import _capi
    return _capi.PK_SEQ_LOSS_GUIDE_ROWS, _capi.PK_SEQ_LOSS_GUIDE_COLS, _capi.PK_SEQ_LOSS_PAIR_TILE, _capi.PK_SEQ_LOSS_F32_CHAIN


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "am_losses.npz")))


def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _guided_case(G, kind):
    """Every (S, T) of the tile-edge grid as one utterance of G maps: list of (G, S, T) float32 arrays (built once, never
    modified)."""
    R, Cc, _, _ = _consts()
    rng = np.random.default_rng(1000 + 10 * G + (kind == "diag"))
    utts = []
    for S in _edges(R):
        for T in _edges(Cc):
            if kind == "softmax":                       # rows of N(0, 1) logits: every row sums to 1
                a = _softmax(rng.standard_normal((G, S, T)))
            else:                                       # sharply diagonal: sum W A is near zero
                d = np.arange(T)[None, :] / T - np.arange(S)[:, None] / S
                a = _softmax(-(d ** 2)[None] / (2 * 0.01 ** 2) + 0.1 * rng.standard_normal((G, S, T)))
            utts.append(a.astype(np.float32))
    return utts


def _pad4(utts):
    B, G = len(utts), utts[0].shape[0]
    S, T = max(u.shape[1] for u in utts), max(u.shape[2] for u in utts)
    T += -T % 4                                         # rows on 16-byte boundaries: the vector loads' path
    a = np.zeros((B, G, S, T), np.float32)
    for b, u in enumerate(utts):
        a[b, :, :u.shape[1], :u.shape[2]] = u
    return a


@pytest.mark.parametrize("kind", ["softmax", "diag"])
@pytest.mark.parametrize("sigma", [0.2, 0.4])
@pytest.mark.parametrize("G", [1, 3, 4])
def test_guided_sums_within_the_derived_bound(G, sigma, kind):
    from parakeet_amd.losses import guided_attention_sums
    chain = _consts()[3]
    utts = _guided_case(G, kind)
    rows, cols = [u.shape[1] for u in utts], [u.shape[2] for u in utts]
    padded = _pad4(utts)
    B, _, Sm, Tm = padded.shape
    want = ar.guided_sums(padded, rows, cols, sigma)
    packed = guided_attention_sums(np.concatenate([u.reshape(-1) for u in utts]), rows, cols, sigma, maps=G)
    rect = guided_attention_sums(padded, rows, cols, sigma, maps=G, offsets=np.arange(B) * (G * Sm * Tm), map_stride=Sm * Tm,
                                 row_stride=Tm)
    assert packed.shape == (B, 2) and packed.dtype == np.float64
    assert np.array_equal(packed, rect)                 # either layout, scalar or 16-byte loads: the same bits
    bound = ar.guided_sums_bound(sigma, want[:, 1], want[:, 0], chain)
    q = np.abs(packed[:, 0] - want[:, 0]) / bound
    qa = np.abs(packed[:, 1] - want[:, 1]) / (2 * ar.U * want[:, 1])
    print(f"SWEEP-RATIO guided_attn G {G} sigma {sigma} {kind}: WA {q.max():.4f} (utterance {int(q.argmax())}: "
          f"{rows[int(q.argmax())]} x {cols[int(q.argmax())]}) A {qa.max():.4f}; smallest sum WA {want[:, 0].min():.3e}")
    assert (q <= 1.0).all() and (qa <= 1.0).all()
    if kind == "diag":
        wide = np.asarray(cols) >= 15                   # enough columns for every row to find its diagonal entry
        assert (want[wide, 0] < 0.05 * want[wide, 1]).all()   # the case a relative bound could not judge


@pytest.mark.parametrize("name,table", [("table_5_5", ac.TABLE_5_5), ("table_3_6", ac.TABLE_3_6)])
def test_guide_entries_are_the_docstring_tables(name, table):
    """One utterance per entry, a one-hot map at (s, t): its sum W A is the guide's entry."""
    from parakeet_amd.losses import guided_attention_sums
    ilen, olen, sigma = ac.TABLES[name]
    hot = np.zeros((olen * ilen, olen, ilen), np.float32)
    for i in range(olen * ilen):
        hot[i, i // ilen, i % ilen] = 1.0
    sums = guided_attention_sums(hot, [olen] * len(hot), [ilen] * len(hot), sigma)
    got = sums[:, 0].reshape(olen, ilen)
    assert np.array_equal(sums[:, 1], np.ones(len(hot)))
    err = np.abs(got - ar.guide(ilen, olen, sigma)).max()
    print(f"SWEEP-RATIO guided_attn entries {name}: {err / ar.guide_entry_bound(sigma):.4f}")
    assert err <= ar.guide_entry_bound(sigma)
    assert np.array_equal(np.round(got, 4), np.asarray(table))
    assert np.abs(got - _gold()[name]).max() <= 2 * ar.guide_entry_bound(sigma)   # the reference's float32 table


def _pair_rows(W):
    tile = _consts()[2]
    rows = [1, 7, 15, 16, 17, 35, 257]
    if W == 1:                                          # the edges of the kernel's own tile of entries
        rows += [tile - 1, tile, tile + 1, 2 * tile + 1]
    return rows


@functools.lru_cache(maxsize=None)
def _pair_case(W):
    rng = np.random.default_rng(2000 + W)
    out = []
    for r in _pair_rows(W):
        t = rng.standard_normal((r, W)).astype(np.float32) * 2 - 6          # raw log-mels: mean -6
        out.append(((t + 0.3 * rng.standard_normal((r, W))).astype(np.float32), t))
    return out


@pytest.mark.parametrize("W", [1, 5, 80, 200])
def test_pair_sums_against_float64_in_both_layouts(W):
    from parakeet_amd.losses import pair_loss_sums
    pairs = _pair_case(W)
    rows = [p.shape[0] for p, _ in pairs]
    d = [p.astype(np.float64) - t.astype(np.float64) for p, t in pairs]
    want = np.array([[np.abs(x).sum(), (x ** 2).sum()] for x in d])
    packed = pair_loss_sums(np.concatenate([p for p, _ in pairs]), np.concatenate([t for _, t in pairs]), rows)
    B, Lp, Lt = len(pairs), max(rows) + 3, max(rows)
    P, T = np.full((B, Lp, W), 7.0, np.float32), np.full((B, Lt, W), -3.0, np.float32)   # padding that would show
    for b, (p, t) in enumerate(pairs):
        P[b, :rows[b]], T[b, :rows[b]] = p, t
    rect = pair_loss_sums(P, T, rows, np.arange(B) * (Lp * W), np.arange(B) * (Lt * W), width=W)
    assert packed.shape == (B, 2) and packed.dtype == np.float64 and np.array_equal(packed, rect)
    # a column block of a wider tensor: row strides above W, odd offsets
    wide_p, wide_t = np.full((B, Lt, W + 3), 9.0, np.float32), np.full((B, Lt, W + 5), 9.0, np.float32)
    for b, (p, t) in enumerate(pairs):
        wide_p[b, :rows[b], 1:W + 1], wide_t[b, :rows[b], 3:W + 3] = p, t
    strided = pair_loss_sums(wide_p, wide_t, rows, np.arange(B) * (Lt * (W + 3)) + 1, np.arange(B) * (Lt * (W + 5)) + 3,
                             pred_stride=W + 3, target_stride=W + 5, width=W)
    assert np.array_equal(packed, strided)
    q = np.abs(packed - want) / (1e-6 * want)
    print(f"SWEEP-RATIO pair_loss W {W}: l1 {q[:, 0].max():.4f} l2 {q[:, 1].max():.4f}")
    assert (q <= 1.0).all()


def _bce_lens():
    tile = _consts()[2]
    return [1, 2, 63, 64, 65, 257, tile - 1, tile, tile + 1, 2 * tile + 1]


@functools.lru_cache(maxsize=None)
def _bce_case():
    rng = np.random.default_rng(3000)
    xs, ys = [], []
    for i, n in enumerate(_bce_lens()):
        x = (3.0 * rng.standard_normal(n)).astype(np.float32)
        y = (rng.random(n) < 0.3).astype(np.float32)
        for j, v in enumerate((30.0, -30.0, 90.0, -90.0)):       # planted where the row has room; a single entry takes turns
            if n >= 4:
                x[(7 * j + 3) % n if n > 4 else j] = v
            elif j == i % 4:
                x[0] = v
        xs.append(x)
        ys.append(y)
    return xs, ys


@pytest.mark.parametrize("pos_weight", [1.0, 5.0])
def test_bce_sums_are_finite_and_match_float64(pos_weight):
    from parakeet_amd.losses import bce_with_logits_sums
    xs, ys = _bce_case()
    lens = [len(x) for x in xs]
    assert {30.0, -30.0, 90.0, -90.0} <= set(np.concatenate(xs).tolist())
    want = np.array([ar.bce_with_logits(x, y, pos_weight).sum() for x, y in zip(xs, ys)])
    got = bce_with_logits_sums(np.concatenate(xs), np.concatenate(ys), lens, pos_weight)
    assert got.shape == (len(lens),) and got.dtype == np.float64 and np.isfinite(got).all()
    L = max(lens)
    X, Y = np.full((len(lens), L), np.nan, np.float32), np.full((len(lens), L), np.nan, np.float32)
    for b, (x, y) in enumerate(zip(xs, ys)):
        X[b, :lens[b]], Y[b, :lens[b]] = x, y
    offs = np.arange(len(lens)) * L
    assert np.array_equal(got, bce_with_logits_sums(X, Y, lens, pos_weight, offs, offs))   # NaN padding is never read
    q = np.abs(got - want) / (1e-6 * np.abs(want))
    print(f"SWEEP-RATIO bce_logits pos_weight {pos_weight}: {q.max():.4f}")
    assert (q <= 1.0).all()


def test_every_entry_point_is_independent_of_the_batch():
    from parakeet_amd.losses import bce_with_logits_sums, guided_attention_sums, pair_loss_sums
    pick = [3, 10, 17, 29, 35]                          # five utterances of different shapes
    utts = [_guided_case(3, "softmax")[i] for i in pick]
    assert len({u.shape for u in utts}) == 5

    def guided(us):
        return guided_attention_sums(np.concatenate([u.reshape(-1) for u in us]), [u.shape[1] for u in us],
                                     [u.shape[2] for u in us], 0.4, maps=3)

    pairs = [_pair_case(80)[i] for i in (0, 2, 4, 5, 6)]

    def pair(ps):
        return pair_loss_sums(np.concatenate([p for p, _ in ps]), np.concatenate([t for _, t in ps]), [len(p) for p, _ in ps])

    xs, ys = _bce_case()
    rows = [(xs[i], ys[i]) for i in (0, 2, 4, 5, 9)]

    def bce(rs):
        return bce_with_logits_sums(np.concatenate([x for x, _ in rs]), np.concatenate([y for _, y in rs]),
                                    [len(x) for x, _ in rs], 5.0)

    for fn, items in ((guided, utts), (pair, pairs), (bce, rows)):
        whole = fn(items)
        for b, it in enumerate(items):
            assert np.array_equal(fn([it])[0], whole[b]), (fn.__name__, b)
        assert np.array_equal(fn(items[::-1])[::-1], whole), fn.__name__
        assert (np.abs(whole) > 0).all()


def test_refusals_and_host_io():
    import ctypes as C
    from parakeet_amd import _capi
    from parakeet_amd.losses import bce_with_logits_sums, guided_attention_sums, pair_loss_sums
    from parakeet_amd.runtime import Context
    a = _guided_case(1, "softmax")[8]
    for sigma in (0.0, -0.4, float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            guided_attention_sums(a, [a.shape[1]], [a.shape[2]], sigma)
    with pytest.raises(ValueError):
        guided_attention_sums(a, [0], [a.shape[2]], 0.4)
    with pytest.raises(ValueError):
        guided_attention_sums(a, [], [], 0.4)
    with pytest.raises(ValueError, match="reaches"):
        guided_attention_sums(a, [a.shape[1] + 1], [a.shape[2]], 0.4)
    with pytest.raises(NotImplementedError):
        pair_loss_sums(np.zeros((1, 8193), np.float32), np.zeros((1, 8193), np.float32), [1])
    with pytest.raises(ValueError):
        pair_loss_sums(np.zeros((2, 4), np.float32), np.zeros((2, 4), np.float32), [])
    with pytest.raises(ValueError, match="pos_weight"):
        bce_with_logits_sums(np.zeros(3, np.float32), np.zeros(3, np.float32), [3], -1.0)
    # host pointers: the same bits as device tensors
    ctx = Context.get()
    i32 = lambda v: np.ascontiguousarray(v, np.int32)   # noqa: E731
    i32p = C.POINTER(C.c_int32)
    out = np.full((1, 2), np.nan)
    G, S, T = a.shape
    _capi.check(ctx.lib.pk_guided_attn_run(ctx.handle, _capi.fptr(a), None, 0, 0, i32([G]).ctypes.data_as(i32p),
                                           i32([S]).ctypes.data_as(i32p), i32([T]).ctypes.data_as(i32p), 1, 0.4,
                                           out.ctypes.data_as(C.c_void_p), _capi.PK_HOST_IO))
    assert np.array_equal(out, guided_attention_sums(a, [S], [T], 0.4))
    p, t = _pair_case(5)[3]
    _capi.check(ctx.lib.pk_pair_loss_run(ctx.handle, _capi.fptr(p), _capi.fptr(t), None, None, 0, 0,
                                         i32([len(p)]).ctypes.data_as(i32p), 1, 5, out.ctypes.data_as(C.c_void_p),
                                         _capi.PK_HOST_IO))
    assert np.array_equal(out, pair_loss_sums(p, t, [len(p)]))
    x, y = (v[3] for v in _bce_case())
    one = np.full(1, np.nan)
    _capi.check(ctx.lib.pk_bce_logits_run(ctx.handle, _capi.fptr(x), _capi.fptr(y), None, None,
                                          i32([len(x)]).ctypes.data_as(i32p), 1, 5.0, one.ctypes.data_as(C.c_void_p),
                                          _capi.PK_HOST_IO))
    assert np.array_equal(one, bce_with_logits_sums(x, y, [len(x)], 5.0))
    rc = ctx.lib.pk_guided_attn_run(ctx.handle, None, None, 0, 0, None, None, None, 1, 0.4, None, 0)
    assert rc == -1 and ctx.lib.pk_last_error()


# ------------------------------------------------------------------------------------------------------ Python surface
def _ok(got, want):
    got = np.asarray([float(v) for v in got] if isinstance(got, (tuple, list)) else float(got), np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape and (np.abs(got - want) <= 2e-6 * np.abs(want)).all(), (got, want)


def _dev0(v):
    assert isinstance(v, torch.Tensor) and v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda


@pytest.mark.parametrize("name", list(ac.FS2_CASES))
def test_fastspeech2_loss_against_the_reference(name):
    from parakeet_amd.fastspeech2 import FastSpeech2Loss
    um, uw, with_after = ac.FS2_CASES[name]
    x = {k: torch.from_numpy(v) for k, v in ac.fs2_inputs().items()}
    if not with_after:
        x["after_outs"] = None
    got = FastSpeech2Loss(use_masking=um, use_weighted_masking=uw)(**x)
    assert len(got) == 4
    for v in got:
        _dev0(v)
    _ok(got, _gold()[name])


@pytest.mark.parametrize("name", list(ac.DUR_CASES))
def test_duration_predictor_loss_against_the_reference(name):
    from parakeet_amd.fastspeech2 import DurationPredictorLoss
    offset, seed = ac.DUR_CASES[name]
    o, t = ac.dur_inputs(seed)
    got = DurationPredictorLoss(offset=offset)(o, t)
    _dev0(got)
    _ok(got, _gold()[name])
    none = DurationPredictorLoss(offset=offset, reduction="none")(o, t)
    assert tuple(none.shape) == o.shape
    _ok(float(none.mean()), _gold()[name])


@pytest.mark.parametrize("name", list(ac.TTS_CASES))
def test_transformer_tts_loss_against_the_reference(name):
    from parakeet_amd.transformer_tts import TransformerTTSLoss
    um, uw, pw = ac.TTS_CASES[name]
    got = TransformerTTSLoss(use_masking=um, use_weighted_masking=uw, bce_pos_weight=pw)(**ac.tts_inputs())
    assert len(got) == 3
    for v in got:
        _dev0(v)
    _ok(got, _gold()[name])


@pytest.mark.parametrize("name", list(ac.GA_CASES))
def test_guided_attention_losses_against_the_reference(name):
    import parakeet_amd.transformer_tts as tts
    cls, sigma, alpha, heads = ac.GA_CASES[name]
    got = getattr(tts, cls)(sigma=sigma, alpha=alpha)(torch.from_numpy(ac.attention(31, heads)), ac.ILENS, ac.OLENS)
    _dev0(got)
    _ok(got, _gold()[name])
    with pytest.raises(ValueError):
        getattr(tts, cls)()(torch.zeros((2, 2) if heads else (1, 2, 2, 2)), [2], [2])


def test_guided_attention_mask_is_the_docstring_table():
    from parakeet_amd.transformer_tts import GuidedAttentionLoss
    for name in ac.TABLES:
        ilen, olen, sigma = ac.TABLES[name]
        m = GuidedAttentionLoss._make_guided_attention_mask(ilen, olen, sigma).numpy()
        assert m.shape == (olen, ilen) and np.abs(m - ar.guide(ilen, olen, sigma)).max() <= ar.guide_entry_bound(sigma)


@pytest.mark.parametrize("name", list(ac.TACO_CASES))
def test_tacotron2_loss_against_the_reference(name):
    from parakeet_amd.tacotron2 import Tacotron2Loss
    stop, guided, sigma = ac.TACO_CASES[name]
    got = Tacotron2Loss(use_stop_token_loss=stop, use_guided_attention_loss=guided, sigma=sigma)(**ac.taco_inputs())
    want = {k.split("/")[1]: v for k, v in _gold().items() if k.startswith(name + "/")}
    assert list(got)[:3] == ["loss", "mel_loss", "post_mel_loss"] and set(got) == set(want)
    for k, v in got.items():
        _dev0(v)
        _ok(v, want[k])


def test_attention_guide_and_guided_attention_loss_against_the_reference():
    from parakeet_amd import losses
    x = ac.taco_inputs()
    att = x["attention_weights"]
    W = losses.attention_guide(torch.from_numpy(ac.OLENS), torch.from_numpy(ac.ILENS), att.shape[1], att.shape[2], ac.GUIDE_G)
    assert W.is_cuda and W.dtype == torch.float32 and tuple(W.shape) == att.shape
    assert np.abs(W.numpy().astype(np.float64) - _gold()["attention_guide"]).max() <= 2 * ar.guide_entry_bound(ac.GUIDE_G)
    got = losses.guided_attention_loss(torch.from_numpy(att), ac.OLENS, ac.ILENS, ac.GUIDE_G)
    _dev0(got)
    _ok(got, _gold()["guided_attention_loss"])


def test_argument_errors():
    from parakeet_amd import synthetic as syn
    from parakeet_amd.fastspeech2 import FastSpeech2Loss
    from parakeet_amd.transformer_tts import TransformerTTS, TransformerTTSLoss
    with pytest.raises(AssertionError):
        FastSpeech2Loss(use_masking=True, use_weighted_masking=True)
    with pytest.raises(AssertionError):
        TransformerTTSLoss(use_masking=True, use_weighted_masking=True)

    def model(**over):
        cfg = dict(syn.TRANSFORMER_TTS_LJSPEECH, elayers=1, dlayers=1, postnet_layers=0, **over)
        m = TransformerTTS(idim=40, odim=80, **cfg)
        m.set_state_dict(syn.transformer_tts_state(40, 80, cfg, seed=41, stop_bias=-6.0))
        return m.eval()

    text, speech = np.ones((1, 4), np.int64), np.zeros((1, 6, 80), np.float32)
    m = model()
    with pytest.raises(TypeError, match="list or tuple"):
        m.evaluate_batch(text, [4], speech, [6], modules_applied_guided_attn="encoder-decoder")
    for mod in ("encoder", "decoder"):
        with pytest.raises(NotImplementedError, match="self-attention"):
            m.evaluate_batch(text, [4], speech, [6], modules_applied_guided_attn=[mod, "encoder-decoder"])
    with pytest.raises(ValueError, match="loss-type"):
        m.evaluate_batch(text, [4], speech, [6], loss_type="L3")
    with pytest.raises(NotImplementedError, match="reduction_factor"):
        model(reduction_factor=2).evaluate_batch(text, [4], speech, [6])
    assert "enc_dec_attn_loss" not in model(reduction_factor=2).evaluate_batch(text, [4], speech, [6],
                                                                                use_guided_attn_loss=False)
