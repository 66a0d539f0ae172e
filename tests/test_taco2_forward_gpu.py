"""Tacotron2 with teacher forcing on the HIP engine (csrc/taco2.hip pk_taco_teacher), through the C ABI: against the
golden vectors of the reference's own ``Tacotron2.forward`` (tools/make_golden_taco_forward.py), against the fp64
restatement (tests/taco2_forward_ref.py), bit for bit against the free-running decode it teacher-forces, and the
``forward`` / ``teacher_forced_batch`` API.  Bars: the project's own for Tacotron2 (tests/test_taco2_gpu.py::_check)."""
import os
import sys

import numpy as np
import pytest
import torch

from parakeet_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import taco2_forward_cases as cases  # noqa: E402
import taco2_forward_ref as fref  # noqa: E402
from ar_cases import T2_CASES  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = cases.KEYS
_SHAPE = {c[0]: c[1] for c in T2_CASES}


def _model(cfg, state, math=None):
    from parakeet_amd.tacotron2 import Tacotron2
    m = Tacotron2(**cfg)
    m.set_state_dict(state)
    m.eval()
    if math:
        m.set_math(math)
    return m


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check(got, ref, name, stop_tol=1e-3):
    """tests/test_taco2_gpu.py::_check, printing each figure before it asserts."""
    for k in KEYS:
        if k not in ref:
            assert k not in got
            continue
        a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        assert a.shape == b.shape, (name, k, a.shape, b.shape)
        d = np.abs(a - b)
        print(f"{name} {k}: mean {d.mean():.3e} max {d.max():.3e}")
        if k == "alignments":
            assert d.max() < 1e-4, (name, k)
        elif k == "stop_logits":
            assert d.max() < stop_tol, (name, k)
        else:
            assert d.mean() < 1e-4 and d.max() < 2e-3, (name, k)


def _small(seed=21, **over):
    cfg = dict(syn.TACOTRON2_LJSPEECH, **dict(_SHAPE["stop"], **over))
    return cfg, syn.tacotron2_state(cfg, seed=seed, stop_bias=-8.0)


def _teacher(rng, L, M=80):
    return (0.5 * rng.standard_normal((L, M))).astype(np.float32)


@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("case", list(cases.CASES))
def test_engine_matches_reference_source(case, math):
    """``forward`` against what the reference's ``Tacotron2.forward`` gave.  In "batch2" the second utterance's
    output_lens is shorter than T_mel: mel_output (zeros included) and the valid rows of alignments / stop_logits compare
    directly; the reference runs its postnet over all T_mel frames before it masks (:762-769), so the valid rows of that
    utterance's mel_outputs_postnet are compared with the engine's pass over all T_mel teacher frames."""
    g = np.load(os.path.join(GOLD, "tacotron2_forward.npz"))
    cfg, u = cases.case_cfg(case), cases.case_inputs(case)
    m = _model(cfg, cases.case_state(case), math)
    B, T = u["ids"].shape
    got = _np(m.forward(u["ids"], np.full(B, T), u["mels"], output_lens=u["output_lens"], tones=u["tones"],
                        global_condition=u["global_condition"], seed=u["seeds"][0]))
    for b in range(B):
        L = u["mels"].shape[1] if u["output_lens"] is None else int(u["output_lens"][b])
        ref = {k: g[f"{case}_{k}"][b] for k in KEYS if f"{case}_{k}" in g.files}
        one = {k: v[b] for k, v in got.items()}
        if L < u["mels"].shape[1]:
            for k in KEYS[:2]:
                assert not np.any(one[k][L:]) and not np.any(ref[k][L:])
            assert not np.any(one["alignments"][L:]) and not np.any(one["stop_logits"][L:])
            full = _np(m.teacher_forced_batch([u["ids"][b]], [u["mels"][b]], seeds=[u["seeds"][b]],
                                              tones=None if u["tones"] is None else [u["tones"][b]])[0])
            assert np.array_equal(full["mel_output"][:L], one["mel_output"][:L])        # causal: the same steps
            one = dict({k: v[:L] for k, v in one.items()}, mel_outputs_postnet=full["mel_outputs_postnet"][:L])
            ref = {k: v[:L] for k, v in ref.items()}
        _check(one, ref, f"{case}[{b}]")
        assert np.abs(one["alignments"].sum(-1) - 1.0).max() < 1e-5


@pytest.mark.parametrize("math", ["f32", "f16x3"])
def test_engine_vs_fp64_restatement_ragged_batch(math):
    """Utterances of different T_b and L_b, each with its own seed, in lockstep: L_b = 1 (the zero query alone), and one
    utterance much longer than the rest (the others keep stepping past their end; nothing of that reaches an output)."""
    cfg, state = _small()
    m = _model(cfg, state, math)
    rng = np.random.default_rng(77)
    Ts, Ls, seeds = (5, 11, 3, 17, 8), (1, 7, 60, 12, 2), [9, 21, 3, 14, 5]
    texts = [rng.integers(1, 37, size=T) for T in Ts]
    mels = [_teacher(rng, L) for L in Ls]
    outs = m.teacher_forced_batch(texts, mels, seeds=seeds)
    assert len(outs) == len(Ts)
    for b, o in enumerate(outs):
        ref = fref.forward(state, texts[b], mels[b], cfg, seed=seeds[b], dtype=torch.float64, return_parts=True)
        enc = ref.pop("encoder_outputs").numpy()
        assert np.abs(m.debug_tap(0, b) - enc).max() < 1e-4
        got = _np(o)
        assert got["mel_output"].shape == (Ls[b], 80) and got["alignments"].shape == (Ls[b], Ts[b])
        assert got["stop_logits"].shape == (Ls[b],)
        _check(got, {k: v.numpy() for k, v in ref.items()}, f"utt{b}")
        assert np.abs(got["alignments"].sum(-1) - 1.0).max() < 1e-5


def _self_consistency(cfg, state, texts, seeds, max_steps, math=None, **kw):
    m = _model(cfg, state, math)
    free = m.infer_batch(texts, max_decoder_steps=max_steps, seeds=seeds, **kw)
    lens = [int(o["mel_output"].shape[0]) for o in free]
    tf = m.teacher_forced_batch(texts, [o["mel_output"] for o in free], seeds=seeds, **kw)     # device tensors
    for b, (a, c) in enumerate(zip(free, tf)):
        a, c = _np(a), _np(c)
        assert set(a) == set(c)
        for k in a:
            assert np.array_equal(a[k], c[k]), (b, k, np.abs(a[k] - c[k]).max())
    host = m.teacher_forced_batch(texts, [o["mel_output"].cpu().numpy() for o in free], seeds=seeds, **kw)   # host arrays
    for a, c in zip(tf, host):
        assert all(np.array_equal(a[k].cpu().numpy(), c[k].cpu().numpy()) for k in a)
    return lens


@pytest.mark.parametrize("math", ["f32", "f16x3"])
def test_teacher_forcing_its_own_output_is_bit_identical(math):
    """infer_batch on a ragged batch that ends at different steps for different reasons, then teacher_forced_batch on its
    own mel_output with the same seeds: every output comes back bit for bit (the precomputed prenet rows are the per-step
    prenet's, the rest of the step is the same kernels on the same operands)."""
    cfg = dict(syn.TACOTRON2_LJSPEECH, **_SHAPE["stop"])
    state = syn.tacotron2_state(cfg, seed=21, stop_bias=-31.4, stop_gain=500.0)
    texts, seeds = [np.load(os.path.join(GOLD, "tacotron2.npz"))["stop_ids"]], [21]
    for k in (7, 20, 14):
        rng = np.random.default_rng(100 + k)
        texts.append(rng.integers(1, 37, size=int(rng.integers(2, 20))))
        seeds.append(k)
    assert _self_consistency(cfg, state, texts, seeds, 40, math) == [29, 2, 40, 40]


def test_self_consistency_other_shapes():
    """The LJSpeech recipe's prenet (80 -> 256 -> 256), no stop token (the content rule ends the free run), tones, and a
    global condition."""
    rng = np.random.default_rng(5)
    cfg = dict(syn.TACOTRON2_LJSPEECH)
    _self_consistency(cfg, syn.tacotron2_state(cfg, seed=25, stop_bias=-8.0), [rng.integers(1, 37, size=T) for T in (12, 5)],
                      [25, 26], 9)
    cfg = dict(syn.TACOTRON2_LJSPEECH, **_SHAPE["nostop"])
    _self_consistency(cfg, syn.tacotron2_state(cfg, seed=22), [rng.integers(1, 37, size=T) for T in (7, 4, 9)], [1, 2, 3], 30)
    cfg = dict(syn.TACOTRON2_LJSPEECH, **_SHAPE["tones"])
    texts = [rng.integers(1, 37, size=T) for T in (8, 3)]
    _self_consistency(cfg, syn.tacotron2_state(cfg, seed=24, stop_bias=-8.0), texts, [4, 5], 6,
                      tones=[rng.integers(0, 5, size=len(t)) for t in texts])
    cfg = dict(syn.TACOTRON2_LJSPEECH, **_SHAPE["global"])
    _self_consistency(cfg, syn.tacotron2_state(cfg, seed=26, stop_bias=-8.0), texts, [6, 7], 5,
                      global_condition=rng.standard_normal((2, 32)).astype(np.float32))


def test_causality():
    """Teacher frame k is the query of step k + 1: outputs and alignments at steps <= k keep their bits, step k + 1 moves;
    the last frame is never a query."""
    cfg, state = _small()
    m = _model(cfg, state)
    rng = np.random.default_rng(8)
    text, mel, k = rng.integers(1, 37, size=9), _teacher(rng, 12), 5
    a = _np(m.teacher_forced_batch([text], [mel], seeds=[3])[0])
    mel2 = mel.copy()
    mel2[k] += 1.0
    b = _np(m.teacher_forced_batch([text], [mel2], seeds=[3])[0])
    for key in ("mel_output", "alignments", "stop_logits"):
        assert np.array_equal(a[key][:k + 1], b[key][:k + 1]), key
    assert np.abs(a["mel_output"][k + 1] - b["mel_output"][k + 1]).max() > 1e-4
    assert np.abs(a["alignments"][k + 1] - b["alignments"][k + 1]).max() > 0
    mel3 = mel.copy()
    mel3[-1] += 1.0
    c = _np(m.teacher_forced_batch([text], [mel3], seeds=[3])[0])
    assert all(np.array_equal(a[key], c[key]) for key in a)


def test_forward_layout_and_batch_independence():
    cfg, state = _small()
    m = _model(cfg, state)
    rng = np.random.default_rng(9)
    B, Tmax, Lmax = 3, 10, 9
    tl, ol = np.array([10, 4, 7]), np.array([6, 9, 1])
    ids = rng.integers(1, 37, size=(B, Tmax))
    mels = (0.5 * rng.standard_normal((B, Lmax, 80))).astype(np.float32)
    out = _np(m.forward(ids, tl, mels, output_lens=ol, seed=40))
    assert out["mel_output"].shape == out["mel_outputs_postnet"].shape == (B, Lmax, 80)
    assert out["alignments"].shape == (B, Lmax, Tmax) and out["stop_logits"].shape == (B, Lmax)
    pieces = m.teacher_forced_batch([ids[b, :tl[b]] for b in range(B)], [mels[b, :ol[b]] for b in range(B)],
                                    seeds=[40, 41, 42])
    for b in range(B):
        L, T = int(ol[b]), int(tl[b])
        p = _np(pieces[b])
        assert np.array_equal(out["mel_output"][b, :L], p["mel_output"])
        assert np.array_equal(out["mel_outputs_postnet"][b, :L], p["mel_outputs_postnet"])
        assert np.array_equal(out["alignments"][b, :L, :T], p["alignments"])
        assert np.array_equal(out["stop_logits"][b, :L], p["stop_logits"])
        for k in KEYS:
            assert not np.any(out[k][b, L:]), (k, b)                              # zeros past output_lens
        assert not np.any(out["alignments"][b, :, T:])
        alone = _np(m.teacher_forced_batch([ids[b, :T]], [mels[b, :L]], seeds=[40 + b])[0])   # alone == inside the batch
        assert all(np.array_equal(alone[k], p[k]) for k in KEYS), b
    # output_lens=None: every utterance uses T_mel frames
    full = _np(m.forward(ids, tl, mels, seed=40))
    ref = m.teacher_forced_batch([ids[b, :tl[b]] for b in range(B)], [mels[b] for b in range(B)], seeds=[40, 41, 42])
    for b in range(B):
        assert np.array_equal(full["mel_outputs_postnet"][b], ref[b]["mel_outputs_postnet"].cpu().numpy())
        assert np.all(np.any(full["mel_output"][b] != 0, axis=-1))
    # torch inputs on the device, B = 1 without the batch axis of the lengths
    dev = m.forward(torch.as_tensor(ids[:1]), torch.as_tensor(tl[:1]), torch.as_tensor(mels[:1]).cuda(), output_lens=ol[:1], seed=40)
    assert np.array_equal(dev["mel_output"].cpu().numpy(), out["mel_output"][:1])


def test_dropout_seed_and_switch():
    cfg, state = _small(seed=5, p_prenet_dropout=0.25)
    m = _model(cfg, state)
    rng = np.random.default_rng(10)
    text, mel = rng.integers(1, 37, size=7), _teacher(rng, 6)
    a = _np(m.teacher_forced_batch([text], [mel], seeds=[1])[0])["mel_output"]
    b = _np(m.teacher_forced_batch([text], [mel], seeds=[2])[0])["mel_output"]
    assert np.array_equal(a, _np(m.teacher_forced_batch([text], [mel], seeds=[1])[0])["mel_output"])
    assert np.abs(a - b).max() > 1e-3                                             # the mask is live
    m.set_dropout(False)
    c = _np(m.teacher_forced_batch([text], [mel])[0])
    ref = fref.forward(state, text, mel, cfg, drop=None, dtype=torch.float64)
    _check(c, {k: v.numpy() for k, v in ref.items()}, "no dropout")


def test_errors_and_state():
    from parakeet_amd import _capi
    from parakeet_amd.tacotron2 import Tacotron2
    cfg, state = _small()
    rng = np.random.default_rng(11)
    text, mel = rng.integers(1, 37, size=6), _teacher(rng, 4)
    fresh = _model(cfg, state)
    fresh._finalize()
    with pytest.raises(RuntimeError):                                             # pk_taco_read before any call
        _capi.check(fresh._ctx.lib.pk_taco_read(fresh._h, None, None, None, None, 0))
    m = _model(cfg, state)
    before = _np(m.infer(text, max_decoder_steps=5, seed=3))
    with pytest.raises(ValueError):
        m.teacher_forced_batch([text], [mel[:, :64]])                             # mel width
    with pytest.raises(ValueError):
        m.teacher_forced_batch([text, text], [mel])                               # count
    with pytest.raises(ValueError):
        m.teacher_forced_batch([text], [mel[:0]])                                 # empty teacher
    with pytest.raises(ValueError):
        m.teacher_forced_batch([np.array([1, 2, 37])], [mel])                     # id out of range, as infer
    with pytest.raises(ValueError):
        m.forward(text[None], [6], mel[None], output_lens=[5])                    # longer than T_mel
    with pytest.raises(ValueError):
        m.forward(text[None], [6], mel[None], output_lens=[0])
    m.teacher_forced_batch([text], [mel], seeds=[3])
    after = _np(m.infer(text, max_decoder_steps=5, seed=3))                       # infer is unchanged after a teacher call
    assert all(np.array_equal(before[k], after[k]) for k in before)
    with pytest.raises(NotImplementedError):
        Tacotron2(**dict(cfg, reduction_factor=2))
    # a model that needs tones / a global condition refuses without, with what infer raises
    tcfg = dict(syn.TACOTRON2_LJSPEECH, **_SHAPE["tones"])
    tm = _model(tcfg, syn.tacotron2_state(tcfg, seed=24, stop_bias=-8.0))
    for call in (lambda: tm.infer(text, max_decoder_steps=3), lambda: tm.teacher_forced_batch([text], [mel])):
        with pytest.raises(ValueError):
            call()
    gcfg = dict(syn.TACOTRON2_LJSPEECH, **_SHAPE["global"])
    gm = _model(gcfg, syn.tacotron2_state(gcfg, seed=26, stop_bias=-8.0))
    gc = rng.standard_normal((1, 32)).astype(np.float32)
    for call in (lambda: gm.infer(text, max_decoder_steps=3), lambda: gm.teacher_forced_batch([text], [mel])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        gm.teacher_forced_batch([text], [mel], global_condition=gc[:, :16])
    gm.teacher_forced_batch([text], [mel], global_condition=gc)
    with pytest.raises(ValueError):                                               # the condition was consumed by that call
        gm.teacher_forced_batch([text], [mel])
    with pytest.raises(ValueError):
        m.teacher_forced_batch([text], [mel], global_condition=gc)                # a model without one


def test_benchmark_size_32_utterances_640_frames():
    """The LJSpeech recipe unshrunk at the size the timing is quoted for: 32 utterances x ~128 tokens x 640 frames in one
    call, two of them (the first, and the last, which is shorter in both) against one fp64 restatement run each."""
    cfg = dict(syn.TACOTRON2_LJSPEECH)
    state = syn.tacotron2_state(cfg, seed=62, stop_bias=-8.0)
    m = _model(cfg, state)
    rng = np.random.default_rng(64)
    Ts = [128] * 31 + [97]
    Ls = [640] * 31 + [577]
    texts = [rng.integers(1, 37, size=T) for T in Ts]
    mels = [_teacher(rng, L) for L in Ls]
    seeds = list(range(100, 132))
    outs = m.teacher_forced_batch(texts, mels, seeds=seeds)
    assert [int(o["mel_output"].shape[0]) for o in outs] == Ls
    for b in (0, 31):
        ref = fref.forward(state, texts[b], mels[b], cfg, seed=seeds[b], dtype=torch.float64)
        got = _np(outs[b])
        _check(got, {k: v.numpy() for k, v in ref.items()}, f"utt{b}")
        assert np.abs(got["alignments"].sum(-1) - 1.0).max() < 1e-5


def test_gta_example_writes_what_teacher_forced_batch_returns(tmp_path):
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location(
        "tacotron2_gta", os.path.join(os.path.dirname(GOLD), "..", "examples", "tacotron2_gta.py"))
    gta = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gta)
    cfg = dict(syn.TACOTRON2_LJSPEECH, **_SHAPE["tones"])
    m = _model(cfg, syn.tacotron2_state(cfg, seed=24, stop_bias=-8.0))
    rng = np.random.default_rng(12)
    rows = []
    for i, (T, L) in enumerate(((6, 9), (11, 4), (3, 7))):
        np.save(tmp_path / f"u{i}.npy", _teacher(rng, L))
        rows.append(dict(utt_id=f"u{i}", text=rng.integers(1, 37, size=T).tolist(), tones=rng.integers(0, 5, size=T).tolist(),
                         mel=f"u{i}.npy"))
    (tmp_path / "metadata.jsonl").write_text("".join(json.dumps(r) + "\n" for r in rows))
    items = gta.read_metadata(str(tmp_path / "metadata.jsonl"))
    gta.run(m, items, str(tmp_path / "out"), seed=50, batch_size=2, save_alignment=True)
    for i, it in enumerate(items):
        ref = m.teacher_forced_batch([it["text"]], [np.load(it["mel"])], tones=[it["tones"]], seeds=[50 + i])[0]
        assert np.array_equal(np.load(tmp_path / "out" / f"u{i}_gta.npy"), ref["mel_outputs_postnet"].cpu().numpy())
        assert np.array_equal(np.load(tmp_path / "out" / f"u{i}_align.npy"), ref["alignments"].cpu().numpy())
